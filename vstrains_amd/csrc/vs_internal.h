// Internal structures and device helpers shared by the HIP translation units.
// gfx950 only: wave = 64 lanes, no other target is considered.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/vstrains_hip.h"
#include "vs_buf.h"
#include "vs_pe_plan.h"  // VsTuning, the probe grid of a read end (vs_seed_phase, vs_seed_probes, VS_SEED_VERIFIED)

#define VS_WAVE 64
#define VS_PAD_WORDS 16  // zero words behind every packed text buffer (window reads may overshoot)

// ---- packed text ---------------------------------------------------------------------------
// 2 bits per base (A=0 C=1 G=2 T=3), 16 bases per uint32 word, base i of a sequence sits in
// word i/16 at bits 2*(i%16) (LSB first).  Every sequence starts on a word boundary and every
// buffer carries VS_PAD_WORDS zero words so that window reads never leave the allocation.

struct VsNodeMeta {
    uint32_t woff;  // first word of the node in fwd_words / rc_words
    uint32_t len;   // bases
};

// One open-address slot of the seed table (16 B, read with one dwordx4 load).
//  key  : canonical w-mer (2w <= 62 bits); bit 62 set = several postings; all ones = empty
//  a, b : single -> a = node, b = pos | (node_strand << 31)
//         multi  -> a = first posting index, b = number of postings
struct VsSlot {
    uint64_t key;
    uint32_t a;
    uint32_t b;
};
#define VS_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull
#define VS_MULTI_BIT (1ull << 62)

// One posting of a seed with several postings (16 B, one dwordx4 load): where the seed lies and
// the header of its node, so that the mapping kernel needs no second round trip for the header.
//   x: node   y: pos [0..23] | strand [31]   z: node length   w: first word of the node text
struct VsPosting {
    uint32_t node, pos, strand, len, woff;
};
#ifdef __HIPCC__
__host__ __device__ inline uint4 vs_posting_pack(const VsPosting &p) {
    uint4 r;
    r.x = p.node;
    r.y = p.pos | (p.strand << 31);
    r.z = p.len;
    r.w = p.woff;
    return r;
}
__host__ __device__ inline VsPosting vs_posting_unpack(const uint4 r) {
    VsPosting p;
    p.node = r.x;
    p.pos = r.y & 0x00FFFFFFu;
    p.strand = r.y >> 31;
    p.len = r.z;
    p.woff = r.w;
    return p;
}
#endif

struct VsIndexDev {
    uint32_t n_nodes;
    uint32_t K;  // split_len = ksize + 1
    uint32_t w;  // seed length (odd, <= 31, <= K)
    uint32_t s;  // probe stride on the read = K - w + 1
    uint32_t table_bits;
    const VsNodeMeta *meta;     // [n_nodes]
    const uint32_t *fwd_words;  // packed node texts
    const uint32_t *rc_words;   // packed reverse complements, same offsets; = fwd_words + rc_delta (one allocation,
    uint32_t rc_delta;          // so that a kernel can address either strand off one uniform base)
    const VsSlot *table;        // [1 << table_bits]
    const uint4 *postings;      // VsPosting records, the postings of one seed contiguous
    const uint32_t *slot_node;  // [1 << table_bits] the locus node of a slot: the node of its first posting as this build stored them (empty slot: anything)
};

struct VsReadsDev {
    uint64_t n_ends;
    const uint32_t *woff;   // [n_ends + 1] word offsets into words
    const uint32_t *meta;   // [n_ends] length (bits 0..23) | flags << 24
    const uint32_t *words;  // packed bases
    const uint32_t *mask;   // same layout, 0b11 at bytes outside ACGT; NULL when no end has any
    const uint32_t *inv4;   // [n_ends] up to four positions (one byte each, 0xFF = none) of such bytes; NULL with mask
};
#define VS_FLAG_N 1u        // read holds an upper-case 'N'
#define VS_FLAG_INVALID 2u  // read holds some other byte outside ACGT
#define VS_FLAG_MANY 4u     // ... more of them than inv4 holds (or one beyond position 254): overflow path
// the slot has no second end (a singles block, vs_reads_pack_single): on an odd end only, with length 0 and no words; the slot is
// classified and counted from its even end alone.  (0x80 is taken on the host: vs_pack_host.h)
#define VS_FLAG_ABSENT 8u
#define VS_LEN_MASK 0x00FFFFFFu
// The length the pair filter (PE_Inference.py:162-165) sees of a SECOND end: an absent one counts as longer than any k+1, so the
// slot is short only if its first end is -- the same compare as for a pair, its mask one bit wider.  (An absent end has no
// other flag, so the N test and the VS_FLAG_MANY test over both ends are the first end's alone as they stand; past the
// filter it is an end of length 0: no seed fits it, so it is never probed, owns no list words and lists 0 nodes.)
#define VS_FILTER_LEN_MASK (VS_LEN_MASK | (VS_FLAG_ABSENT << 24))

// ---- host-side objects -----------------------------------------------------------------------
// pinned staging of one FASTQ block in flight (vs_fastq_block): packed words (+ pad), word offsets,
// lengths | flags; two sets alternate, the cores fill one while the other is still being uploaded
struct FqStage {
    VsPinnedBuf words, woff, meta;
    hipEvent_t done = nullptr;  // the uploads out of this set have finished
    bool in_flight = false;
};

void vs_tuning_load(VsTuning &t, bool experiment);  // production (false): the defaults

struct vs_ctx {
    int device = 0;
    bool experiment = false;   // VS_EXPERIMENT=1 at vs_ctx_create: the test hooks of VsTuning exist
    VsTuning tune;
    // vs_ctx_keep_masks: every read block built from now on keeps its validity mask, so that the depth pass (vs_node_depth),
    // which counts the ends the PE filter drops too, sees where their 'N's are (without it a block whose only bytes outside
    // ACGT are 'N's gives its mask back, vs_reads_finish, and the mapped ingest packs on the host without one)
    bool keep_masks = false;
    // vs_contig_mems: the match records of the last pass (grow-only, kept for the copy-out call), the scan of the ends'
    // probe counts, the scan's block sums with the probe total and the record count behind them
    VsDevBuf d_mems, d_mem_scan, d_mem_tmp;
    uint64_t mems_info[4] = {0, 0, 0, 0};  // records, launches of k_contig_mems, probes, capacity in records before the pass
    // vs_cover_layout / vs_cover_fold: the exclusive scan of the difference array (one word per slot) and the scans' block sums
    VsDevBuf d_cover_scan, d_cover_tmp;
    // vs_node_indels: the record count of the pass and its four tallies, added to the caller's only when the pass fit
    VsDevBuf d_indel_tmp;
    hipStream_t stream = nullptr;
    std::string err;
    FqStage fq_stage[2];
    unsigned fq_next = 0;
    bool has_index = false;
    VsIndexDev idx{};
    // owned device allocations of the index
    VsDevBuf d_meta, d_fwd, d_table, d_post, d_slot_node;
    uint64_t n_seed_pos = 0, n_slots = 0, n_distinct = 0, index_bytes = 0;
    uint32_t max_node_len = 0;
    // scratch for vs_pe_count
    VsDevBuf d_slow_list;          // pair indices sent to the slow path
    VsDevBuf d_slow_count;         // SC_WORDS uint32 counters, zeroed before every count
    enum SlowCount : uint32_t {
        SC_MID = 0,         // pairs for k_pe_mid
        SC_ACC_QUEUE = 1,   // k_pe_accumulate's chunk queue
        SC_SLOW = 8,        // pairs for k_pe_slow
        SC_STRIP_QUEUE = 9, // k_rows_sum's strip queue
        SC_OWNERS = 15,     // owning ends
        SC_WORDS = 16       // (the other words unused)
    };
    VsDevBuf links_spare;          // vs_links_reserve: the buffer of the next link table (links_spare_n nodes)
    uint32_t links_spare_n = 0;
    VsDevBuf d_slow_list2;         // pairs k_pe_mid hands on to k_pe_slow
    VsDevBuf d_dense;              // dense per-workgroup state for the slow path
    uint32_t dense_nodes = 0xFFFFFFFFu;  // node count the dense layout was initialised for
    // locus order scratch (k_pe_locus / k_pe_permute)
    VsDevBuf d_locus_keys, d_perm, d_locus_hist, d_scan_tmp;
    double last_sort_ms = 0;
    // per-end accepted lists between k_pe_tiles and k_pe_accumulate
    VsDevBuf d_lists, d_list_counts;
    // row-owner counting (k_list_owners / k_rows_count / k_rows_fill / k_rows_sum): per matrix and row the counts, cursors
    // and offsets (6 x (N + 2) words), the items of every row (one word per listed node), the multiplicity of every end's list
    VsDevBuf d_rows, d_row_entries, d_mult, d_ltab;
    // grow-only device scratch slots of the graph-stage entry points (no allocation per call)
    VsDevBuf scratch[32];
    // device buffers of freed read blocks, kept for the next block of about the same size (the
    // FASTQ ingest makes and frees one block per million pairs)
    struct CachedBuf { VsDevBuf buf; bool used; };
    std::vector<CachedBuf> cache;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double last_ms[3] = {0, 0, 0};
    const char *last_kernel = "";  // mapping-kernel instantiation of the last vs_pe_count
    uint32_t last_launched = 0;    // VS_RAN_* bits: which optional kernels that call launched
    uint64_t last_order_pairs = 0; // pairs of that call (vs_pe_last_order: d_locus_keys / d_perm hold their order if a sort ran)
    // the hand-off of that call, if it made one (vs_pe_last_handoff: d_lists / d_list_counts / d_slow_list hold it): pairs (0 = none),
    // end slots, ends per tile, layout, table slots and list trim of the k_pe_tiles instantiation that ran
    struct LastHandoff { uint64_t pairs = 0, list_ends = 0; uint32_t ept = 0, rows = 0, pool = 0, trim = 0; } last_handoff;
    // the overflow kernels of that call, if it launched them (vs_pe_last_overflow: d_slow_count / d_slow_list2 hold what they left):
    // pairs (0 = none), whether k_pe_mid was skipped
    struct LastOverflow { uint64_t pairs = 0; uint32_t no_mid = 0; } last_overflow;
    int n_cu = 256;
};

struct vs_reads {
    uint64_t n_ends = 0, n_words = 0, max_len = 0, n_invalid = 0, bytes = 0;
    // the five arrays as the kernels see them, all from one place: lent by the context's cache (cached: the blocks of the
    // FASTQ ingests, one after another of about the same size) or held by the block itself in own[]
    void *d_woff = nullptr, *d_meta = nullptr, *d_words = nullptr, *d_mask = nullptr, *d_inv4 = nullptr;
    bool cached = false;
    bool unpaired = false;  // a singles block: every odd end is VS_FLAG_ABSENT (all slots are singles, or none are)
    VsDevBuf own[5];
    hipError_t alloc(vs_ctx *ctx, void *&view, size_t bytes);  // one more array (vs_reads.hip)
    void release(vs_ctx *ctx, void *&view);                    // ... given back; view = NULL
    VsReadsDev dev() const {
        VsReadsDev r;
        r.n_ends = n_ends;
        r.woff = (const uint32_t *)d_woff;
        r.meta = (const uint32_t *)d_meta;
        r.words = (const uint32_t *)d_words;
        r.mask = (const uint32_t *)d_mask;
        r.inv4 = (const uint32_t *)d_inv4;
        return r;
    }
};

int vs_fail(vs_ctx *ctx, int code, const char *fmt, ...);
extern "C" void vs_ctx_free_index(vs_ctx *ctx);
#define VS_HIP(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess)                                                             \
            return vs_fail(ctx, e__ == hipErrorOutOfMemory ? VS_E_OOM : VS_E_HIP,          \
                           "%s failed: %s", #call, hipGetErrorString(e__));                \
    } while (0)

// UTF-8 checks of the FASTQ ingest (vs_fastq.hip), shared with the streamed ingest (vs_stream.hip): the characters that
// start in [lo, hi) of txt[0, size) are valid; bytes of the character at q[0] (n available), 0 if invalid
bool vs_utf8_range_ok(const uint8_t *txt, size_t size, size_t lo, size_t hi);
uint32_t vs_utf8_char_len(const uint8_t *q, size_t n);
// host threads a parallel host loop may use (the affinity mask cut by the cgroup quota, or VS_HOST_THREADS): vs_fastq.hip
unsigned vs_host_threads();
// How a read block comes to be (vs_reads.hip), for every builder, on the stream the builder works on.
// The arrays of block r, from where r->cached says: woff and meta for n_ends ends at the first call; words (and the mask
// beside them, where asked) once n_words is known -- in the same call or a later one -- with their pad tails zeroed.
// Sets n_ends, n_words and bytes.
hipError_t vs_reads_alloc(vs_ctx *ctx, hipStream_t st, vs_reads *r, uint64_t n_ends, const uint64_t *n_words, bool with_mask);
// The last step of a block packed on the device, its mask written: the ends flagged VS_FLAG_INVALID counted into *d_cnt
// (zero before) and read back through *h_cnt (synchronises st) = n_invalid; none: the mask goes back; else it stays, inv4 is
// built from it and bytes grows by both.
hipError_t vs_reads_finish(vs_ctx *ctx, hipStream_t st, vs_reads *r, uint32_t *d_cnt, uint32_t *h_cnt);
// A window of the streamed ingest (vs_stream.hip): its text and the byte offsets of its n_nl line ends
struct SlWin {
    const uint8_t *txt;
    const uint32_t *ends;
    uint32_t n_nl, size;
};
// exclusive scan of a[0, m) in place by one workgroup (k_sl_scan of vs_stream.hip); the total, below 2^32, to *total
void vs_launch_scan_u32(hipStream_t st, uint32_t *a, uint32_t m, uint32_t *total);
// The ends of a block of the BAM ingest (vs_bam.hip): end e is record ends[e] of recs (n_rec of them; BamRec of vs_bam_core.h:
// four words, the flag in the low 16 bits of the second, l_seq the third, the offset of the 4-bit bases in win the fourth)
struct BamEnds {
    const uint8_t *win;
    const uint32_t *recs;
    const uint32_t *ends;
    uint32_t n_rec;
};
// The kept singletons of the BAM ingest (VS_BAM_BY_NAME_KEEP): a singles block whose even end e is record list[e / 2] of recs
// (as BamEnds), every odd end absent
struct BamSingles {
    const uint8_t *win;
    const uint32_t *recs;
    const uint32_t *list;
    uint32_t n_rec;
};
// THE way a streamed ingest cuts a block of n_ends ends out of its device window (vs_reads.hip, one entry per source of ends;
// a singles source gives a block with vs_reads::unpaired): wcnt reserved, the block's woff and meta, k_block_ends<Src> (lengths,
// word counts), the scan, woff copied, ONE read-back and wait, words and mask, k_pack_reads<Src>, vs_reads_finish, the last wait.
// d_st / h_st: n_st >= VS_BLK_ST status words on the device / pinned.  The first VS_BLK_ST are rewritten here; the words behind
// them are the caller's, set by a kernel of its own on st before the call, and come back in the same read-back.
// hipSuccess with *out == NULL: h_st[VS_BLK_BAD] names the first end that stops the block -- e | VS_BLK_OVER: longer than
// VS_LEN_MASK; e alone: its source has no such record (PackPairs, PackBam, PackBamSingles test their lists) -- the caller words it.
enum { VS_BLK_MAXLEN = 0, VS_BLK_BAD = 1 /* ~0u: none */, VS_BLK_WORDS = 2, VS_BLK_INVALID = 3, VS_BLK_ST = 4 };
#define VS_BLK_OVER 0x80000000u
struct VsBlockJob {
    vs_ctx *ctx;
    hipStream_t st;
    uint64_t n_ends;  // <= 2^31
    VsDevBuf *wcnt;   // scratch of the caller, grown here
    uint32_t *d_st, *h_st, n_st;
    bool more;        // the caller has work for st behind the block and waits for both itself: no last wait here
};
hipError_t vs_block_lines(const VsBlockJob &j, const SlWin &f0, const SlWin &f1, vs_reads **out);  // end e: record e / 2 of window e & 1
hipError_t vs_block_records(const VsBlockJob &j, const SlWin &w, const uint32_t *rec, vs_reads **out);  // record rec[e] of ONE window
hipError_t vs_block_singles(const VsBlockJob &j, const SlWin &w, const uint32_t *rec, uint32_t first, vs_reads **out);  // even e: rec[e / 2], or first + e / 2 (rec NULL)
hipError_t vs_block_pairs(const VsBlockJob &j, const SlWin &f0, uint32_t n_rec0, const SlWin &f1, uint32_t n_rec1, const uint32_t *rec, vs_reads **out);  // rec[e] of window e & 1
hipError_t vs_block_bam(const VsBlockJob &j, const BamEnds &b, vs_reads **out);
hipError_t vs_block_bam_singles(const VsBlockJob &j, const BamSingles &b, vs_reads **out);

// BGZF members (vs_inflate.hip), shared with the streamed ingest.  A member for the device: its raw deflate payload in a
// buffer of compressed bytes, where its ISIZE bytes go in an output buffer, and the CRC32 of its trailer.
struct vs_bgzf_member {
    uint32_t in_off, in_len, out_off, isize, crc;
};
// p[0, avail): 0 when a whole BGZF member starts at p (*m with in_off relative to p and out_off 0, *member_size its bytes),
// 1 when what is there may still become one with more bytes, 2 when it is not BGZF
int vs_bgzf_parse(const uint8_t *p, size_t avail, vs_bgzf_member *m, size_t *member_size);
// the same verdict from the header alone: *header_size = the bytes in front of the payload, *member_size = all of the member
int vs_bgzf_header(const uint8_t *p, size_t avail, size_t *header_size, size_t *member_size);
// n members, one wavefront each: status[i] = 0 or an INF_E_* word; atomicMin(first_bad, base + i) for every i that failed
// (member i is dir[i], or dir[n - 1 - i] when `reversed`)
void vs_launch_inflate(hipStream_t st, const uint8_t *comp, uint64_t comp_size, uint8_t *out, uint64_t out_size, const vs_bgzf_member *dir,
                       uint32_t n, uint32_t *status, uint32_t *first_bad, uint32_t base, int reversed);
// n members counted and thrown away (k_inflate_count): `grid` wavefronts, each with 64 KiB of `scratch` of its own, loop
// over the members; res[4 i ..] = status, newlines, flags (bit 0 '\r', bit 1 a byte >= 0x80), last byte of member dir[i]
void vs_launch_inflate_count(hipStream_t st, const uint8_t *comp, uint64_t comp_size, uint8_t *scratch, uint32_t grid, const vs_bgzf_member *dir,
                             uint32_t n, uint32_t *res);
// the same decoder on the host (vs_inflate_core.h with one lane): the status word
uint32_t vs_inflate_member_host(const uint8_t *pay, uint32_t len, uint8_t *out, uint32_t isize, uint32_t crc);

// BGZF members made on the device (vs_deflate.hip).  text[0, text_bytes) is cut into n = ceil(text_bytes / 0xFF00) members,
// one wavefront each: member i lies at slots[i * stride, + sizes[i]) and may use `cap` <= stride bytes of its slot
// (cap >= 0xFF00 + 31 always suffices); res[2 i] = 0 or a DEF_E_* word (sizes[i] is then 0), res[2 i + 1] = 0 stored /
// 1 fixed / 2 dynamic
void vs_launch_deflate(hipStream_t st, const uint8_t *text, uint64_t text_bytes, uint32_t n, uint8_t *slots, uint64_t slots_bytes, uint32_t stride,
                       uint32_t cap, uint32_t *sizes, uint32_t *res);
// member i's sizes[i] bytes from its slot to packed[offs[i] ...) (offs: the exclusive scan of sizes); nothing beyond packed_bytes
void vs_launch_deflate_pack(hipStream_t st, const uint8_t *slots, uint32_t stride, const uint32_t *sizes, const uint32_t *offs, uint32_t n,
                            uint8_t *packed, uint64_t packed_bytes);
// the same encoder on the host (vs_deflate_core.h with one lane): the DEF_* status word
uint32_t vs_deflate_member_host(const uint8_t *text, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *size, uint32_t *kind);
extern const uint8_t vs_bgzf_eof[28];  // the empty member that ends a BGZF file

#define VS_LINKS_SPARSE_MIN 32768u  // nodes from which a table with a dirty-tile map is held as CSR rows (4 GiB of counters)
// The pieces of vs_links_from_cells (vs_graph.hip), shared with vs_links_from_info (vs_info_read.hip).
// A dense table of n nodes, its cells zeroed on the ctx stream: the buffer vs_links_reserve set aside, or a new one.
int vs_links_dense_zeroed(vs_ctx *ctx, const char *who, uint32_t n, vs_links **out, int64_t **d_p0);
// host cells uploaded and added to a dense table: P0[r][c] += v and, off the diagonal, P0[c][r] += v; synchronises the stream
int vs_links_scatter_cells(vs_ctx *ctx, int64_t *d_p0, uint32_t n, const uint32_t *rows, const uint32_t *cols, const int64_t *vals, uint64_t n_cells);
// the CSR table of host cells (every cell and its mirror, equal cells merged, sums of zero dropped)
int vs_links_csr_from_cells(vs_ctx *ctx, const uint32_t *rows, const uint32_t *cols, const int64_t *vals, uint64_t n_cells, uint32_t n, vs_links **out);
// a table that is not handed out after all: a dense buffer goes back to where vs_links_reserve keeps it
void vs_links_abandon(vs_ctx *ctx, vs_links *L);

// Exclusive scan of n uint32 values on the ctx stream (in -> out, may alias); total (uint64) is
// written to d_total if not NULL.  tmp must hold ceil(n/2048)+1 uint64.
int vs_scan_u32(vs_ctx *ctx, const uint32_t *in, uint32_t *out, uint64_t n, uint64_t *d_tmp,
                uint64_t *d_total);

// ---- device helpers ----------------------------------------------------------------------------
#ifdef __HIPCC__

__device__ __forceinline__ uint32_t vs_code(uint8_t c) {
    // A C G T -> 0 1 2 3, anything else -> 4
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// 32 bases (64 bits) starting at base offset `base` of a packed word array.
__device__ __forceinline__ uint64_t vs_win64(const uint32_t *w, uint64_t base) {
    uint64_t i = base >> 4;
    uint32_t sh = (uint32_t)(base & 15u) * 2u;
    uint64_t lo = (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
    uint64_t hi = (uint64_t)w[i + 2];
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

// Same with a 32-bit base offset (LDS tiles, node texts below 2^32 bases): no 64-bit address math.
__device__ __forceinline__ uint64_t vs_win64_u32(const uint32_t *w, uint32_t base) {
    const uint32_t i = base >> 4;
    const uint32_t sh = (base & 15u) * 2u;
    const uint32_t w0 = w[i], w1 = w[i + 1], w2 = w[i + 2];
    // funnel shifts: (w1:w0) >> sh and (w2:w1) >> sh, sh in 0..30
    const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh);
    const uint32_t hi = __builtin_amdgcn_alignbit(w2, w1, sh);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

__device__ __forceinline__ uint64_t vs_win(const uint32_t *w, uint32_t base) { return vs_win64_u32(w, base); }
__device__ __forceinline__ uint64_t vs_win(const uint32_t *w, uint64_t base) { return vs_win64(w, base); }

// x / d with a precomputed magic = floor(2^32 / d) + 1 (0 stands for d == 1); exact while
// x * d < 2^32, which holds for the tile-sized operands used here
__device__ __forceinline__ uint32_t vs_fastdiv(uint32_t x, uint32_t magic) { return magic ? __umulhi(x, magic) : x; }

__device__ __forceinline__ uint64_t vs_lowmask(uint32_t bits) {  // bits in 0..64
    return bits >= 64u ? ~0ull : ((1ull << bits) - 1ull);
}

// Reverse complement of a w-mer held LSB-first in the low 2w bits.
__device__ __forceinline__ uint64_t vs_rc(uint64_t x, uint32_t w) {
    // order of the 2-bit codes reversed = all 64 bits reversed (two v_bfrev_b32), then the two bits of
    // every code swapped back; complement = bitwise not
    x = __builtin_bitreverse64(x);
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    return (~x) >> (64u - 2u * w);
}

__device__ __forceinline__ uint64_t vs_mix64(uint64_t z);
// Key of the seed (w-mer, w <= 63) at base offset `base` of a packed text, and which strand it is the smaller on.
// w <= 31: the canonical w-mer itself.  Longer seeds (k >= 95: w = 63) do not fit a 62-bit key: the key is a mix of the
// canonical 2w bits, so two different seeds may share a key -- which is why, for those indexes, the comparison that
// follows a probe starts at the seed's FIRST base instead of behind it (VS_SEED_VERIFIED below): a posting is credited
// on compared text only, the key merely nominates it.
template <typename B>
__device__ __forceinline__ uint64_t vs_seed_key(const uint32_t *words, B base, uint32_t w, uint32_t *strand) {
    if (w <= 31u) {
        const uint64_t f = vs_win(words, base) & vs_lowmask(2u * w);
        const uint64_t r = vs_rc(f, w);
        *strand = r < f ? 1u : 0u;
        return r < f ? r : f;
    }
    const uint32_t sh = 2u * (w - 32u);  // bits of the seed in the second word pair (w = 63: 62)
    const uint64_t lo = vs_win(words, base), hi = vs_win(words, base + (B)32) & vs_lowmask(sh);
    // reverse complement of the 2w bits (hi:lo): the first 32 bases reversed go to the top
    const uint64_t rl = vs_rc(lo, 32u), rh = vs_rc(hi, w - 32u);
    const uint64_t rc_lo = (rl << sh) | rh, rc_hi = sh ? rl >> (64u - sh) : 0ull;
    const bool rev = rc_hi < hi || (rc_hi == hi && rc_lo < lo);
    *strand = rev ? 1u : 0u;
    const uint64_t a = rev ? rc_lo : lo, b = rev ? rc_hi : hi;
    return vs_mix64(a ^ vs_mix64(b + 0x632BE59BD9B4E019ull)) >> 2;  // 62 bits: neither the empty key nor the multi flag
}
// does the seed at `base` hold a byte outside ACGT?  (mask: 0b11 per such byte)
template <typename B>
__device__ __forceinline__ bool vs_seed_dirty(const uint32_t *mask, B base, uint32_t w) {
    if (w <= 32u) return (vs_win(mask, base) & vs_lowmask(2u * w)) != 0ull;
    return vs_win(mask, base) != 0ull || (vs_win(mask, base + (B)32) & vs_lowmask(2u * (w - 32u))) != 0ull;
}

__device__ __forceinline__ uint32_t vs_slot_of(uint64_t key, uint32_t bits) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64u - bits));
}

__device__ __forceinline__ uint64_t vs_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// index of the last element <= x in a sorted array a[0..n) with a[0] <= x
template <typename T>
__device__ __forceinline__ uint32_t vs_upper_idx(const T *a, uint32_t n, T x) {
    uint32_t lo = 0, hi = n;  // invariant: a[lo] <= x, a[hi] > x (virtually)
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Inclusive scans over the 64 lanes of a wavefront by DPP moves -- row_shr 1, 2, 4, 8 inside the rows of 16 lanes, then the
// last lane of a row broadcast to the rows after it (row_bcast 15 / 31) -- six VALU instructions where the __shfl_up form
// takes six ds_bpermute round trips through the LDS crossbar (r6).  A lane whose source lies outside its row keeps the `old`
// operand: the identity of the operation.
#define VS_DPP_STEP(op, ctrl, rowmask) { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rowmask, 0xf, false); v = op; }
__device__ __forceinline__ uint32_t vs_wave_scan_add(uint32_t v) {
    VS_DPP_STEP(v + t_, 0x111, 0xf) VS_DPP_STEP(v + t_, 0x112, 0xf) VS_DPP_STEP(v + t_, 0x114, 0xf) VS_DPP_STEP(v + t_, 0x118, 0xf)
    VS_DPP_STEP(v + t_, 0x142, 0xa) VS_DPP_STEP(v + t_, 0x143, 0xc)
    return v;
}
__device__ __forceinline__ uint32_t vs_wave_scan_max(uint32_t v) {
    VS_DPP_STEP(v > t_ ? v : t_, 0x111, 0xf) VS_DPP_STEP(v > t_ ? v : t_, 0x112, 0xf) VS_DPP_STEP(v > t_ ? v : t_, 0x114, 0xf)
    VS_DPP_STEP(v > t_ ? v : t_, 0x118, 0xf) VS_DPP_STEP(v > t_ ? v : t_, 0x142, 0xa) VS_DPP_STEP(v > t_ ? v : t_, 0x143, 0xc)
    return v;
}

#endif  // __HIPCC__
