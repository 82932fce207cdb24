// Read pairs from one collated BAM file: the streamed ingest of vs_stream.hip with a different way to find the records.
//
// Host: the Reader of vs_stream_reader.h fills its ring with whole BGZF members and k_inflate (vs_inflate.hip) inflates them
// into the window, CRC32 checked, exactly as for BGZF FASTQ.  Only the header is looked at on the host: vs_bam_header
// inflates the leading members with zlib until magic, text and references are consumed and hands the device the number of
// inflated bytes to skip (it may be larger than a window).
//
// Device: the window starts at a record boundary.  A record is block_size = le32(p) and block_size bytes, so the record
// starts are a serial chain; they are found exactly, from the known start, in three passes (vs_bam_core.h):
//   k_bam_exits    a workgroup per segment of `seg` bytes: next(p) of every byte into LDS, pointer doubling until every
//                  entry has left the segment (next is strictly forward, so any value read while another lane writes it is
//                  still a point of the same chain), then 2 bytes per window byte to memory;
//   k_bam_walk     one lane: from the start through the tables, one lookup per segment the chain touches; the entry
//                  offset of each such segment, how and where the chain ends;
//   k_bam_count    one thread per segment with an entry walks its records (tens of them): records, and records that take part;
//   (k_sl_scan)    both counts to offsets;
//   k_bam_scatter  the same walk: offset, flag and class, l_seq and sequence offset of every record at its index, the
//                  index of every record that takes part at its compacted index; the first malformed record by atomicMin;
// and per block of n couples
//   k_bam_couples  couple c = compacted records 2c, 2c + 1: one first and one second or the first bad couple by atomicMin;
//                  the forward and the reverse record of every couple, the cut;
//   the block builder (vs_block_bam, vs_reads.hip), as every block of a streamed ingest is built: lengths, word offsets, packing;
//   k_bam_tally    records seen and dropped, by class, among those the block passes.
// No kernel waits for another workgroup; every window read and LDS index is tested against its range.
//
// The window is scanned once per appended chunk; blocks are cut from the scanned records with a cursor.  The carry is
// everything from the first record not delivered: an odd record, or the record the window's end cuts.
//
// By name (VS_BAM_BY_NAME): the mates of a pair may lie anywhere in the file.  A window is then [the records still waiting
// for their mates, whole, in file order][new bytes]; the chain passes run over it as above (carried records are ordinary
// records) and the participating records are joined on their names (the rule and every step: vs_bam_core.h):
//   k_mate_hash     a lane per participating record: 64-bit hash of its name;
//   k_mate_claim    open-address table of participating indices in device memory, claimed by atomicCAS, names compared
//                   byte for byte out of the window; the record pushes itself on its name's list (atomicExch);
//   k_mate_rank     a bounded walk of the name's list: rank within the own class, paired or waiting, bytes to carry;
//   k_mate_partner  the same walk for the partner; the later record of a pair emits it;
//   (k_sl_scan)     per workgroup: emitters, waiting records and their bytes to bases (a word per 256 records);
//   k_mate_emit     the place inside the workgroup by a prefix over its lanes: the pair list (first, second) in the order of
//                   the emitting record, the waiting list, the offset of every waiting record among the carried bytes;
//   the block builder on a block of pairs from that list with a cursor: the list is the ends (k_bam_couples takes neighbours);
//   k_mate_carry    a wavefront per waiting record copies it to the front of the other window buffer, 16 bytes a lane
//                   where source and destination are aligned alike; the bytes from `stop` on follow.
// No lane waits for another lane's progress: a lost compare-and-swap reads the winner and goes on.
// What still waits at the end of the input are singletons: counted, and under VS_BAM_BY_NAME_KEEP handed out from the last
// window's waiting list (window order = file order) as singles blocks by the same builder (vs_block_bam_singles: even end e =
// waiting record e / 2, reversed and complemented under 0x10; odd ends absent).
//
// A member range (vs_bam_stream_open_range; one process per GPU on one collated whole-BGZF file).  A range cannot be entered
// at a guessed record start, so the open has two passes with one exchange between them (pe.BamStream.open_shard):
//   vs_bam_share_summary  the rank's members and the few behind them that hold 64 inflated bytes, window by window through
//                         the reader, k_inflate, k_bam_exits_cnt (exits with the count of participating records) and
//                         k_bam_lanes (a lane per candidate start, position and count carried across windows): per candidate
//                         where the chain leaves the share and what it counted (the rule: vs_bam_core.h); the text is not kept;
//   vs_bam_shard_plan     from every rank's summary each rank's true entry, the participating records in front of it, where
//                         its ownership ends -- or why rank 0 reads the whole file instead;
//   the ranged stream     this stream from the range's first member: the bytes in front of the entry dropped as the header is,
//                         the previous rank's second record passed over when the count in front is odd, k_bam_owned for the
//                         records that start below the end of the ownership (couples whose first record does are delivered,
//                         those records are counted), members behind that end inflated one at a time until the last second
//                         record is whole.  Messages name a record by its byte offset in the inflated file.
#include "vs_stream_reader.h"
#include "vs_stream_window.h"
#include "vs_bam_core.h"

#define BAM_TPB 256

namespace {

enum {
    B_END = 0,      // BAM_END_* of the walk
    B_STOP = 1,     // where
    B_NREC = 2,
    B_NPART = 3,
    B_BLOCK = 4,      // the VS_BLK_ST words of the block builder; behind them, read back with them, k_bam_couples' three:
    B_BADCOUPLE = 8,  // first couple of the block that is not one first and one second, ~0u: none
    B_CUT = 9,        // offset of the first record behind the block
    B_CUTREC = 10,    // ... and its index
    B_MALFORMED = 11, // index of the first malformed record, ~0u: none
    B_BAD_MEMBER = 12,  // first BGZF member the device rejected (a running index), ~0u: none
    B_OWN_REC = 13,     // a ranged stream: records / participating records of the window that this rank owns
    B_OWN_PART = 14,
    B_TALLY = 16,       // + class: records passed so far (cumulative)
    B_ALL = 24
};

}  // namespace

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BAM_TPB) k_bam_exits(const uint8_t *__restrict__ win, uint64_t n, uint32_t seg, uint16_t *__restrict__ tab) {
    extern __shared__ uint32_t e[];  // seg words: below 2^31 the offset in the segment the chain goes to next, else 2^31 | exit code
    __shared__ uint32_t changed;
    constexpr uint32_t T = 0x80000000u;
    const uint64_t lo = (uint64_t)blockIdx.x * seg;
    if (lo >= n) return;
    const uint64_t hi = lo + seg < n ? lo + seg : n;
    const uint32_t len = (uint32_t)(hi - lo);
    for (uint32_t i = threadIdx.x; i < len; i += BAM_TPB) {
        uint64_t nx = 0;
        const int st = bam_step(win, n, lo + i, &nx);
        e[i] = st == BAM_STEP_NEED ? T | (uint32_t)BAM_X_NEED : st == BAM_STEP_DEAD ? T | (uint32_t)BAM_X_DEAD
               : nx >= hi ? T | bam_exit_encode(nx, hi) : (uint32_t)(nx - lo);
    }
    __syncthreads();
    for (;;) {
        if (threadIdx.x == 0) changed = 0u;
        __syncthreads();
        bool mine = false;
        for (uint32_t i = threadIdx.x; i < len; i += BAM_TPB) {
            const uint32_t v = e[i];
            if (v & T) continue;
            const uint32_t w = v < len ? e[v] : T | (uint32_t)BAM_X_DEAD;  // (v < len always: it came from nx < hi)
            e[i] = w;
            mine = mine || !(w & T);
        }
        if (mine) changed = 1u;
        __syncthreads();
        const bool again = changed != 0u;
        __syncthreads();
        if (!again) break;
    }
    for (uint32_t i = threadIdx.x; i < len; i += BAM_TPB) tab[lo + i] = (uint16_t)(e[i] & 0xFFFFu);
}

__global__ void __launch_bounds__(VS_WAVE) k_bam_walk(const uint8_t *__restrict__ win, uint64_t n, const uint16_t *__restrict__ tab, uint32_t seg,
                                                      uint64_t start, uint32_t *__restrict__ entry, uint32_t *__restrict__ st) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t stop = 0;
    st[B_END] = (uint32_t)bam_walk(win, n, tab, seg, start, entry, &stop);
    st[B_STOP] = (uint32_t)stop;
}

__global__ void __launch_bounds__(BAM_TPB) k_bam_count(const uint8_t *__restrict__ win, uint64_t n, uint32_t seg, uint32_t n_seg,
                                                       const uint32_t *__restrict__ entry, uint32_t *__restrict__ cnt_rec, uint32_t *__restrict__ cnt_part) {
    const uint32_t s = blockIdx.x * BAM_TPB + threadIdx.x;
    if (s >= n_seg) return;
    uint32_t nr = 0, np = 0;
    if (entry[s] != BAM_NONE) {
        const uint64_t lo = (uint64_t)s * seg, hi = lo + seg < n ? lo + seg : n;
        uint64_t p = entry[s], at = 0;
        while (bam_seg_next(win, n, hi, &p, &at)) {
            nr++;
            if ((bam_classify(win, at).flag_cls >> 16) <= (uint32_t)BAM_C_SECOND) np++;
        }
    }
    cnt_rec[s] = nr;
    cnt_part[s] = np;
}

__global__ void __launch_bounds__(BAM_TPB) k_bam_scatter(const uint8_t *__restrict__ win, uint64_t n, uint32_t seg, uint32_t n_seg,
                                                         const uint32_t *__restrict__ entry, const uint32_t *__restrict__ base_rec,
                                                         const uint32_t *__restrict__ base_part, uint32_t n_rec, uint32_t n_part,
                                                         uint4 *__restrict__ recs, uint32_t *__restrict__ part, uint32_t *__restrict__ st) {
    const uint32_t s = blockIdx.x * BAM_TPB + threadIdx.x;
    if (s >= n_seg || entry[s] == BAM_NONE) return;
    const uint64_t lo = (uint64_t)s * seg, hi = lo + seg < n ? lo + seg : n;
    uint64_t p = entry[s], at = 0;
    uint32_t ri = base_rec[s], pi = base_part[s];
    while (bam_seg_next(win, n, hi, &p, &at)) {
        const BamRec r = bam_classify(win, at);
        const uint32_t cls = r.flag_cls >> 16;
        if (ri < n_rec) recs[ri] = make_uint4(r.off, r.flag_cls, r.l_seq, r.seq_off);
        if (cls == (uint32_t)BAM_C_MALFORMED) atomicMin(&st[B_MALFORMED], ri);
        if (cls <= (uint32_t)BAM_C_SECOND) {
            if (pi < n_part) part[pi] = ri;
            pi++;
        }
        ri++;
    }
}

// one thread per couple of the block: the check, which record is which end, and (thread 0) the cut behind the block
__global__ void __launch_bounds__(BAM_TPB) k_bam_couples(const uint4 *__restrict__ recs, const uint32_t *__restrict__ part, uint32_t part0, uint32_t n_pairs,
                                                         uint32_t n_rec, uint32_t stop, uint32_t *__restrict__ ends, uint32_t *__restrict__ st) {
    const uint32_t c = blockIdx.x * BAM_TPB + threadIdx.x;
    if (c == 0 && n_pairs) {
        const uint32_t after = part[part0 + 2u * n_pairs - 1u] + 1u;
        st[B_CUTREC] = after;
        st[B_CUT] = after < n_rec ? recs[after].x : stop;
    }
    if (c >= n_pairs) return;
    const uint32_t a = part[part0 + 2u * c], b = part[part0 + 2u * c + 1u];
    const uint32_t fa = recs[a].y, fb = recs[b].y;
    if (!bam_couple_ok(fa, fb)) atomicMin(&st[B_BADCOUPLE], c);
    const bool a_first = (fa >> 16) == (uint32_t)BAM_C_FIRST;  // (the first is the forward end)
    ends[2u * c] = a_first ? a : b;
    ends[2u * c + 1u] = a_first ? b : a;
}

__global__ void __launch_bounds__(BAM_TPB) k_bam_tally(const uint4 *__restrict__ recs, uint32_t from, uint32_t to, uint32_t *__restrict__ tally) {
    const uint32_t i = from + blockIdx.x * BAM_TPB + threadIdx.x;
    const uint32_t cls = i < to ? recs[i].y >> 16 : 0xFFu;
#pragma unroll
    for (uint32_t k = 0; k <= (uint32_t)BAM_C_MALFORMED; k++) {
        const unsigned long long b = __ballot(cls == k);
        if ((threadIdx.x & (VS_WAVE - 1u)) == 0 && b) atomicAdd(&tally[k], (uint32_t)__popcll(b));
    }
}


// ---- the summary of a share (vs_bam_core.h) ---------------------------------------------------------------------------------
// k_bam_exits with a count: a sibling, so that the kernel of the whole-file stream stays as it is.  The word of byte i is
// 2^31 (terminal) | participating records << 16 | the offset in the segment the chain goes to next, or the exit code.  The
// invariant of a word: "the chain from i reaches that point after that many participating records that start in front of
// it".  A lane's update is ONE 32-bit store computed from two 32-bit loads, its own word (i -> o after a) and the word of
// o (o -> t after b), and gives i -> t after a + b: any two words that hold the invariant compose to one that holds it, so
// whatever another lane has made of the word of o by the time it is read -- every store is a whole consistent word -- the
// result is a point of the same chain with its own count, as in k_bam_exits.  A segment holds at most seg / 36 < 2^15
// records, so the sum never reaches bit 31.  Tables for [0, lim), lim <= n: segments are clipped to lim.
__global__ void __launch_bounds__(BAM_TPB) k_bam_exits_cnt(const uint8_t *__restrict__ win, uint64_t n, uint64_t lim, uint32_t seg,
                                                           uint16_t *__restrict__ tab, uint16_t *__restrict__ cnt) {
    extern __shared__ uint32_t e[];
    __shared__ uint32_t changed;
    constexpr uint32_t T = 0x80000000u, CNT = 0x7FFF0000u;
    const uint64_t lo = (uint64_t)blockIdx.x * seg;
    if (lo >= lim || lim > n) return;
    const uint64_t hi = lo + seg < lim ? lo + seg : lim;
    const uint32_t len = (uint32_t)(hi - lo);
    for (uint32_t i = threadIdx.x; i < len; i += BAM_TPB) {
        uint64_t nx = 0;
        uint32_t part = 0;
        const int st = bam_step_cnt(win, n, lo + i, &nx, &part);
        e[i] = st == BAM_STEP_NEED ? T | (uint32_t)BAM_X_NEED : st == BAM_STEP_DEAD ? T | (uint32_t)BAM_X_DEAD
               : nx >= hi ? T | (part << 16) | bam_exit_encode(nx, hi) : (part << 16) | (uint32_t)(nx - lo);
    }
    __syncthreads();
    for (;;) {
        if (threadIdx.x == 0) changed = 0u;
        __syncthreads();
        bool mine = false;
        for (uint32_t i = threadIdx.x; i < len; i += BAM_TPB) {
            const uint32_t v = e[i];
            if (v & T) continue;
            const uint32_t o = v & 0xFFFFu;
            const uint32_t w = o < len ? e[o] : T | (uint32_t)BAM_X_DEAD;  // (o < len always: it came from nx < hi)
            e[i] = (w & ~CNT) | (((v & CNT) + (w & CNT)) & CNT);
            mine = mine || !(w & T);
        }
        if (mine) changed = 1u;
        __syncthreads();
        const bool again = changed != 0u;
        __syncthreads();
        if (!again) break;
    }
    for (uint32_t i = threadIdx.x; i < len; i += BAM_TPB) {
        tab[lo + i] = (uint16_t)(e[i] & 0xFFFFu);
        cnt[lo + i] = (uint16_t)((e[i] & CNT) >> 16);
    }
}

// a lane per candidate through the window's tables (bam_lane_walk: bounded by the window's segments, no lane waits for another)
__global__ void __launch_bounds__(BAM_TPB) k_bam_lanes(const uint8_t *__restrict__ win, uint64_t n, uint64_t lim, const uint16_t *__restrict__ tab,
                                                       const uint16_t *__restrict__ cnt, uint32_t seg, uint64_t base, BamLane *__restrict__ lanes,
                                                       uint32_t n_lanes) {
    const uint32_t i = blockIdx.x * BAM_TPB + threadIdx.x;
    if (i >= n_lanes || lim > n) return;
    BamLane l = lanes[i];
    bam_lane_walk(win, n, lim, tab, cnt, seg, base, &l);
    lanes[i] = l;
}

// ownership of a ranged stream: st[B_OWN_REC] / st[B_OWN_PART] = the records / participating records of the scanned window
// that start below `lim` (records lie in the order of their offsets; both words are 0 before)
__global__ void __launch_bounds__(BAM_TPB) k_bam_owned(const uint4 *__restrict__ recs, const uint32_t *__restrict__ part, uint32_t n_rec, uint32_t n_part,
                                                       uint32_t lim, uint32_t *__restrict__ st) {
    const uint32_t i = blockIdx.x * BAM_TPB + threadIdx.x;
    if (i < n_rec && recs[i].x < lim && (i + 1u == n_rec || recs[i + 1u].x >= lim)) st[B_OWN_REC] = i + 1u;
    if (i < n_part) {
        const uint32_t r = part[i], nx = i + 1u < n_part ? part[i + 1u] : n_rec;
        if (r < n_rec && recs[r].x < lim && (nx >= n_rec || recs[nx].x >= lim)) st[B_OWN_PART] = i + 1u;
    }
}

// ---- mates by name ----------------------------------------------------------------------------------------------------------
namespace {
enum { M_NPAIRS = 0, M_NWAIT = 1, M_WBYTES = 2, M_CROWDED = 3 /* ~record, 0xFFFFFFFF: none (atomicMin) */, M_BAD = 4, M_ALL = 8 };
}

__global__ void __launch_bounds__(BAM_TPB) k_mate_hash(BamMates m, uint64_t n, uint32_t bits, uint32_t *__restrict__ st) {
    const uint32_t i = blockIdx.x * BAM_TPB + threadIdx.x;
    if (i >= m.n_part) return;
    uint64_t h = 0;
    const uint32_t r = bam_mate_rec(m, i);
    const uint64_t off = r == BAM_NONE ? n : (uint64_t)m.recs[4u * r];
    if (off + 36u > n || off + 36u + m.win[off + 12u] > n) atomicOr(&st[M_BAD], 1u);  // (never: the scan found the record whole)
    else h = bam_name_hash(m.win, (uint32_t)off, bits);
    m.hash[i] = h;
}

__global__ void __launch_bounds__(BAM_TPB) k_mate_claim(BamMates m, uint32_t *__restrict__ st) {
    const uint32_t i = blockIdx.x * BAM_TPB + threadIdx.x;
    if (i >= m.n_part || st[M_BAD]) return;  // (M_BAD: a record index out of range, nothing is followed)
    const uint32_t s = bam_mate_claim(m, i);
    if (s == BAM_NONE) atomicOr(&st[M_BAD], 2u);
    bam_mate_push(m, i, s);
}

// exclusive prefix of v over the workgroup's BAM_TPB threads, every thread calls; *total: the workgroup's sum
__device__ inline uint32_t bam_block_excl(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const uint32_t lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t o = 1; o < VS_WAVE; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == VS_WAVE - 1u) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < BAM_TPB / VS_WAVE; w++) {
        if (w < wave) base += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();  // (wsum is free for the next call)
    *total = tot;
    return base + inc - v;
}

// wbytes: 4 + block_size for a record that goes on waiting, else 0
__global__ void __launch_bounds__(BAM_TPB) k_mate_rank(BamMates m, uint32_t *__restrict__ wbytes, uint32_t *__restrict__ st) {
    const uint32_t i = blockIdx.x * BAM_TPB + threadIdx.x;
    if (i >= m.n_part || st[M_BAD]) return;  // (M_BAD: a record index out of range, nothing is followed)
    bool crowded = false;
    const uint32_t rk = bam_mate_rank(m, i, &crowded);
    if (crowded) atomicMin(&st[M_CROWDED], ~m.part[i]);  // (the complement: the newest record of a crowded name wins)
    m.rank[i] = rk;
    wbytes[i] = (rk & BAM_MATE_PAIRED) ? 0u : 4u + bam_le32(m.win + bam_mate_off(m, i));
}

// partner[i]: the earlier record of the pair i completes, BAM_NONE when i completes none.  Per workgroup: the pairs its
// records complete, its waiting records and their bytes (sums[0 / 1 / 2][blockIdx.x]; scanned, they are the bases of k_mate_emit)
__global__ void __launch_bounds__(BAM_TPB) k_mate_partner(BamMates m, uint32_t *__restrict__ partner, const uint32_t *__restrict__ wbytes,
                                                          uint32_t *__restrict__ sum_e, uint32_t *__restrict__ sum_w, uint32_t *__restrict__ sum_b,
                                                          const uint32_t *__restrict__ st) {
    __shared__ uint32_t wsum[BAM_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * BAM_TPB + threadIdx.x;
    if (st[M_BAD]) return;  // (the same for every thread)
    uint32_t e = 0, w = 0, b = 0;
    if (i < m.n_part) {
        uint32_t j = BAM_NONE;
        const bool paired = (m.rank[i] & BAM_MATE_PAIRED) != 0u;
        if (paired) j = bam_mate_partner(m, i);
        const bool emits = j < i;  // (BAM_NONE is above every index)
        partner[i] = emits ? j : BAM_NONE;
        e = emits ? 1u : 0u;
        w = paired ? 0u : 1u;
        b = wbytes[i];
    }
    uint32_t te, tw, tb;
    bam_block_excl(e, wsum, &te);
    bam_block_excl(w, wsum, &tw);
    bam_block_excl(b, wsum, &tb);
    if (threadIdx.x == 0) {
        sum_e[blockIdx.x] = te;
        sum_w[blockIdx.x] = tw;
        sum_b[blockIdx.x] = tb;
    }
}

// sum_e / sum_w / sum_b scanned: the workgroup's bases; the place inside the workgroup by the same prefix.  pairs[2 p] = the
// first, [2 p + 1] = the second of the pair emitter i completes; wlist[w] = record, wpart[w] = participating index of the
// w-th waiting record; woff[i]: 4 + block_size of a waiting record in, its offset among the carried bytes out
__global__ void __launch_bounds__(BAM_TPB) k_mate_emit(BamMates m, const uint32_t *__restrict__ partner, const uint32_t *__restrict__ sum_e,
                                                       const uint32_t *__restrict__ sum_w, const uint32_t *__restrict__ sum_b, uint32_t n_pairs, uint32_t n_wait,
                                                       uint32_t *__restrict__ pairs, uint32_t *__restrict__ wlist, uint32_t *__restrict__ wpart,
                                                       uint32_t *__restrict__ woff) {
    __shared__ uint32_t wsum[BAM_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * BAM_TPB + threadIdx.x;  // (launched only when the status words are clean)
    const bool in = i < m.n_part;
    const uint32_t j = in ? partner[i] : BAM_NONE;
    const bool emits = in && j < i, waits = in && !(m.rank[i] & BAM_MATE_PAIRED);
    const uint32_t bytes = waits ? woff[i] : 0u;
    uint32_t t;
    const uint32_t p = sum_e[blockIdx.x] + bam_block_excl(emits ? 1u : 0u, wsum, &t);
    const uint32_t w = sum_w[blockIdx.x] + bam_block_excl(waits ? 1u : 0u, wsum, &t);
    const uint32_t o = sum_b[blockIdx.x] + bam_block_excl(bytes, wsum, &t);
    if (emits && p < n_pairs) {
        const bool i_first = bam_mate_cls(m, i) == (uint32_t)BAM_C_FIRST;
        pairs[2u * p] = m.part[i_first ? i : j];
        pairs[2u * p + 1u] = m.part[i_first ? j : i];
    }
    if (waits && w < n_wait) {
        wlist[w] = m.part[i];
        wpart[w] = i;
        woff[i] = o;
    }
}

// a wavefront per waiting record: its 4 + block_size bytes to dst + woff[its participating index]
__global__ void __launch_bounds__(BAM_TPB) k_mate_carry(BamMates m, uint64_t n, const uint32_t *__restrict__ wpart, uint32_t n_wait,
                                                        const uint32_t *__restrict__ woff, uint8_t *__restrict__ dst, uint64_t dst_size) {
    const uint32_t w = (blockIdx.x * BAM_TPB + threadIdx.x) / VS_WAVE, lane = threadIdx.x & (VS_WAVE - 1u);
    if (w >= n_wait) return;
    const uint32_t i = wpart[w];
    if (i >= m.n_part) return;
    const uint64_t off = bam_mate_off(m, i), to = woff[i];
    if (off + 4u > n) return;
    const uint64_t len = 4ull + bam_le32(m.win + off);
    if (off + len > n || to + len > dst_size) return;
    const uint8_t *s = m.win + off;
    uint8_t *t = dst + to;
    uint64_t head = len, body = 0;
    if ((((uintptr_t)s ^ (uintptr_t)t) & 15u) == 0u) {  // aligned alike: bytes up to a 16-byte boundary, 16 bytes a lane, the rest
        head = (16u - ((uintptr_t)t & 15u)) & 15u;
        if (head > len) head = len;
        body = (len - head) >> 4;
    }
    for (uint64_t k = lane; k < head; k += VS_WAVE) t[k] = s[k];
    const uint4 *s16 = (const uint4 *)(s + head);
    uint4 *t16 = (uint4 *)(t + head);
    for (uint64_t k = lane; k < body; k += VS_WAVE) t16[k] = s16[k];
    for (uint64_t k = head + 16u * body + lane; k < len; k += VS_WAVE) t[k] = s[k];
}

// ---- the chain on a device window ---------------------------------------------------------------------------------------
namespace {

// the segment length to use: `seg` clamped, the default for 0 -- or, where 0 means the environment, what VS_BAM_SEG says (tests:
// records across segments)
uint32_t seg_checked(uint32_t seg, bool zero_is_env = false) {
    if (seg == 0 && zero_is_env)
        if (const char *ev = getenv("VS_BAM_SEG")) seg = (uint32_t)atoll(ev);
    return seg == 0 ? BAM_SEG_DEFAULT : std::min<uint32_t>(std::max<uint32_t>(seg, BAM_SEG_MIN), BAM_SEG_MAX);
}

struct BamScan {
    VsDevBuf tab, entry, cnt_rec, cnt_part, recs, part;
    uint32_t n_rec = 0, n_part = 0, end = BAM_END_CLEAN, stop = 0, malformed = BAM_NONE;
};

// the records of win[0, n) on the chain from `start`, on stream st; d_stat / h_stat: B_ALL words each (synchronises st)
int bam_scan_device(vs_ctx *ctx, hipStream_t st, const uint8_t *win, uint64_t n, uint64_t start, uint32_t seg, BamScan &sc, uint32_t *d_stat,
                    uint32_t *h_stat) {
    const uint64_t n_seg64 = (n + seg - 1u) / seg;
    if (n > STREAM_MAX_WINDOW || n_seg64 > 0x7FFFFFFFu) return vs_fail(ctx, VS_E_RANGE, "a BAM window of %llu bytes", (unsigned long long)n);
    const uint32_t n_seg = (uint32_t)n_seg64;
    sc.n_rec = sc.n_part = 0;
    sc.end = BAM_END_CLEAN;
    sc.stop = (uint32_t)n;
    sc.malformed = BAM_NONE;
    VS_HIP(ctx, hipMemsetAsync(d_stat, 0, sizeof(uint32_t) * B_BAD_MEMBER, st));
    VS_HIP(ctx, hipMemsetAsync(d_stat + B_MALFORMED, 0xFF, sizeof(uint32_t), st));
    if (n_seg) {
        if (int rc = reserve_n<uint16_t>(ctx, sc.tab, n)) return rc;
        if (int rc = reserve_n<uint32_t>(ctx, sc.entry, n_seg)) return rc;
        if (int rc = reserve_n<uint32_t>(ctx, sc.cnt_rec, (size_t)n_seg + 1u)) return rc;
        if (int rc = reserve_n<uint32_t>(ctx, sc.cnt_part, (size_t)n_seg + 1u)) return rc;
        VS_HIP(ctx, hipMemsetAsync(sc.entry.ptr(), 0xFF, sizeof(uint32_t) * n_seg, st));
        const unsigned grid = (n_seg + BAM_TPB - 1u) / BAM_TPB;
        hipLaunchKernelGGL(k_bam_exits, dim3(n_seg), dim3(BAM_TPB), sizeof(uint32_t) * seg, st, win, n, seg, sc.tab.as<uint16_t>());
        VS_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_bam_walk, dim3(1), dim3(VS_WAVE), 0, st, win, n, sc.tab.as<const uint16_t>(), seg, start, sc.entry.as<uint32_t>(), d_stat);
        VS_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_bam_count, dim3(grid), dim3(BAM_TPB), 0, st, win, n, seg, n_seg, sc.entry.as<const uint32_t>(), sc.cnt_rec.as<uint32_t>(),
                           sc.cnt_part.as<uint32_t>());
        VS_HIP(ctx, hipGetLastError());
        vs_launch_scan_u32(st, sc.cnt_rec.as<uint32_t>(), n_seg, d_stat + B_NREC);
        VS_HIP(ctx, hipGetLastError());
        vs_launch_scan_u32(st, sc.cnt_part.as<uint32_t>(), n_seg, d_stat + B_NPART);
        VS_HIP(ctx, hipGetLastError());
    }
    VS_HIP(ctx, hipMemcpyAsync(h_stat, d_stat, sizeof(uint32_t) * B_ALL, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    if (!n_seg) return VS_OK;
    sc.n_rec = h_stat[B_NREC];
    sc.n_part = h_stat[B_NPART];
    sc.end = h_stat[B_END];
    sc.stop = h_stat[B_STOP];
    if (int rc = reserve_n<uint4>(ctx, sc.recs, (size_t)sc.n_rec + 1u)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, sc.part, (size_t)sc.n_part + 1u)) return rc;
    if (sc.n_rec) {
        hipLaunchKernelGGL(k_bam_scatter, dim3((n_seg + BAM_TPB - 1u) / BAM_TPB), dim3(BAM_TPB), 0, st, win, n, seg, n_seg, sc.entry.as<const uint32_t>(),
                           sc.cnt_rec.as<const uint32_t>(), sc.cnt_part.as<const uint32_t>(), sc.n_rec, sc.n_part, sc.recs.as<uint4>(), sc.part.as<uint32_t>(),
                           d_stat);
        VS_HIP(ctx, hipGetLastError());
        VS_HIP(ctx, hipMemcpyAsync(h_stat + B_MALFORMED, d_stat + B_MALFORMED, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
        sc.malformed = h_stat[B_MALFORMED];
    }
    return VS_OK;
}

// couples [part0 / 2, part0 / 2 + n_pairs) of a scanned window: the record of every end (ends), d_stat[B_BADCOUPLE] (~0u before),
// d_stat[B_CUT] and [B_CUTREC]
void launch_ends(hipStream_t st, const BamScan &sc, uint32_t part0, uint32_t n_pairs, uint32_t *ends, uint32_t *d_stat) {
    hipLaunchKernelGGL(k_bam_couples, dim3((n_pairs + BAM_TPB - 1u) / BAM_TPB), dim3(BAM_TPB), 0, st, sc.recs.as<const uint4>(), sc.part.as<const uint32_t>(),
                       part0, n_pairs, sc.n_rec, sc.stop, ends, d_stat);
}

// the match of a scanned window
struct BamMatch {
    VsDevBuf hash, table, slot, next, rank, partner, woff, sums, pairs, wlist, wpart, stat;
    uint32_t n_pairs = 0, n_wait = 0, wait_bytes = 0, crowded = BAM_NONE;
    BamMates view = {};
};

// the pairs and the waiting records of the scanned window win[0, n) on stream st (synchronises it).  mt.crowded: the newest
// record of a name with more than BAM_MATE_CAP records of one class (then there are no lists), else BAM_NONE.
int bam_match_device(vs_ctx *ctx, hipStream_t st, const uint8_t *win, uint64_t n, const BamScan &sc, uint32_t bits, BamMatch &mt) {
    mt.n_pairs = mt.n_wait = mt.wait_bytes = 0;
    mt.crowded = BAM_NONE;
    const uint32_t np = sc.n_part;
    if (!np) return VS_OK;
    if (np > 0x3FFFFFFFu) return vs_fail(ctx, VS_E_RANGE, "%u records to match by name in one window", np);
    const uint32_t size = bam_table_size(np);
    if (int rc = reserve_n<uint64_t>(ctx, mt.hash, np)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, mt.table, 2u * (size_t)size)) return rc;
    for (VsDevBuf *b : {&mt.slot, &mt.next, &mt.rank, &mt.partner, &mt.woff})
        if (int rc = reserve_n<uint32_t>(ctx, *b, (size_t)np + 1u)) return rc;
    const uint32_t n_wg = (np + BAM_TPB - 1u) / BAM_TPB;
    if (int rc = reserve_n<uint32_t>(ctx, mt.sums, 3u * (size_t)n_wg)) return rc;
    uint32_t *sum_e = mt.sums.as<uint32_t>(), *sum_w = sum_e + n_wg, *sum_b = sum_w + n_wg;
    if (int rc = reserve_n<uint32_t>(ctx, mt.stat, M_ALL)) return rc;
    uint32_t *d_ms = mt.stat.as<uint32_t>(), h_ms[M_ALL];
    BamMates &m = mt.view;
    m.win = win;
    m.recs = (const uint32_t *)sc.recs.as<uint4>();
    m.part = sc.part.as<const uint32_t>();
    m.n_rec = sc.n_rec;
    m.n_part = np;
    m.hash = mt.hash.as<uint64_t>();
    m.table = mt.table.as<uint32_t>();
    m.head = m.table + size;
    m.size = size;
    m.slot = mt.slot.as<uint32_t>();
    m.next = mt.next.as<uint32_t>();
    m.rank = mt.rank.as<uint32_t>();
    VS_HIP(ctx, hipMemsetAsync(d_ms, 0, sizeof(uint32_t) * M_ALL, st));
    VS_HIP(ctx, hipMemsetAsync(d_ms + M_CROWDED, 0xFF, sizeof(uint32_t), st));
    VS_HIP(ctx, hipMemsetAsync(m.table, 0xFF, sizeof(uint32_t) * 2u * (size_t)size, st));
    const dim3 grid(n_wg), tpb(BAM_TPB);
    hipLaunchKernelGGL(k_mate_hash, grid, tpb, 0, st, m, n, bits, d_ms);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_mate_claim, grid, tpb, 0, st, m, d_ms);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemsetAsync(sum_e, 0, sizeof(uint32_t) * 3u * (size_t)n_wg, st));
    hipLaunchKernelGGL(k_mate_rank, grid, tpb, 0, st, m, mt.woff.as<uint32_t>(), d_ms);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_mate_partner, grid, tpb, 0, st, m, mt.partner.as<uint32_t>(), mt.woff.as<const uint32_t>(), sum_e, sum_w, sum_b, d_ms);
    VS_HIP(ctx, hipGetLastError());
    vs_launch_scan_u32(st, sum_e, n_wg, d_ms + M_NPAIRS);  // (a word per workgroup: the places inside one are found in k_mate_emit)
    VS_HIP(ctx, hipGetLastError());
    vs_launch_scan_u32(st, sum_w, n_wg, d_ms + M_NWAIT);
    VS_HIP(ctx, hipGetLastError());
    vs_launch_scan_u32(st, sum_b, n_wg, d_ms + M_WBYTES);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(h_ms, d_ms, sizeof(uint32_t) * M_ALL, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    if (h_ms[M_BAD]) return vs_fail(ctx, VS_E_STATE, "matching by name: %s", (h_ms[M_BAD] & 1u) ? "a record index beyond the window's records" : "the name table is full");
    if (h_ms[M_CROWDED] != BAM_NONE) {
        mt.crowded = ~h_ms[M_CROWDED];
        return VS_OK;
    }
    mt.n_pairs = h_ms[M_NPAIRS];
    mt.n_wait = h_ms[M_NWAIT];
    mt.wait_bytes = h_ms[M_WBYTES];
    if (int rc = reserve_n<uint32_t>(ctx, mt.pairs, 2u * (size_t)mt.n_pairs + 1u)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, mt.wlist, (size_t)mt.n_wait + 1u)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, mt.wpart, (size_t)mt.n_wait + 1u)) return rc;
    hipLaunchKernelGGL(k_mate_emit, grid, tpb, 0, st, m, mt.partner.as<const uint32_t>(), sum_e, sum_w, sum_b, mt.n_pairs, mt.n_wait, mt.pairs.as<uint32_t>(),
                       mt.wlist.as<uint32_t>(), mt.wpart.as<uint32_t>(), mt.woff.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// the waiting records of a matched window win[0, n) to dst[0, wait_bytes), in window order
int bam_carry_device(vs_ctx *ctx, hipStream_t st, uint64_t n, const BamMatch &mt, uint8_t *dst, uint64_t dst_size) {
    if (!mt.n_wait) return VS_OK;
    const uint64_t threads = (uint64_t)mt.n_wait * VS_WAVE;
    hipLaunchKernelGGL(k_mate_carry, dim3((unsigned)((threads + BAM_TPB - 1u) / BAM_TPB)), dim3(BAM_TPB), 0, st, mt.view, n, mt.wpart.as<const uint32_t>(), mt.n_wait,
                       mt.woff.as<const uint32_t>(), dst, dst_size);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

void fill_info(uint64_t info[6], uint64_t n_rec, uint64_t n_part, uint32_t end, uint64_t stop, uint32_t malformed, uint32_t bad_couple) {
    info[0] = n_rec;
    info[1] = n_part;
    info[2] = end;
    info[3] = stop;
    info[4] = malformed == BAM_NONE ? ~0ull : malformed;
    info[5] = bad_couple == BAM_NONE ? ~0ull : bad_couple;
}

}  // namespace

// ---- the stream ------------------------------------------------------------------------------------------------------------
struct vs_bam_stream : StreamState {  // (B_ALL status words)
    int device = 0;
    hipStream_t st = nullptr;
    Reader rd;
    DevWindow w;  // inflated BAM bytes that start at a record boundary
    bool eof = false;
    uint64_t skip = 0;  // header bytes still to drop from the front
    uint32_t seg = BAM_SEG_DEFAULT;
    BamScan sc;
    bool scanned = false;
    uint32_t rec_cur = 0, part_cur = 0;  // the first record / compacted record of the scanned window not yet delivered
    uint64_t first_record = 0;           // file-wide number of the window's record 0
    VsDevBuf d_wcnt, d_ends;
    uint64_t pairs = 0;
    // by name
    bool by_name = false;
    uint32_t name_bits = 64;
    BamMatch mt;
    uint32_t pair_cur = 0;   // the first pair of the matched window not yet delivered
    bool keep = false;       // VS_BAM_BY_NAME_KEEP: what still waits at the end of the input is handed out as singles blocks
    uint32_t single_cur = 0; // ... the first waiting record of the last window not yet delivered
    uint32_t n_carried = 0;  // the window's first records are the ones carried from earlier windows (first_record: its first NEW one)
    uint64_t singletons = 0, waiting_max = 0, carried_bytes_max = 0, windows = 0;
    // a member range (vs_bam_stream_open_range): positions are relative to S, the inflated offset of the range's first member
    bool ranged = false;
    uint64_t share_start = 0;      // S, for messages
    uint64_t own_end = ~0ull;      // records that start at or behind it are the next rank's (~0: the end of the file)
    bool skip_part = false;        // the first participating record is the second of the previous rank's last couple
    uint64_t win_base = 0;         // position of the window's byte 0
    uint64_t read_pos = 0;         // position of the next member to inflate
    uint32_t own_rec = 0, own_part = 0;  // of the scanned window: its records / participating records below own_end
    SlotLease held;                // the slot whose members are being inflated, the next one is held_at
    uint32_t held_at = 0;
};

namespace {

// (rec: index in the window; the records carried in front of the new ones have been numbered before)
std::string rec_msg(const vs_bam_stream *s, uint64_t rec, const char *what) {
    if (s->ranged) {  // (no file-wide number: the record's offset in the inflated file, fetched from the scanned window)
        uint32_t off = s->sc.stop;
        if (rec < s->sc.n_rec) (void)hipMemcpy(&off, (const uint32_t *)(s->sc.recs.as<uint4>() + rec), sizeof off, hipMemcpyDeviceToHost);
        return s->rd.path + ": the record at byte " + std::to_string(s->share_start + s->win_base + off) + " of the inflated file (a member range: records are named by offset)" + what;
    }
    return s->rd.path + ": record " + std::to_string(s->first_record + rec - std::min<uint64_t>(rec, s->n_carried)) + what;
}

const char *NOT_COLLATED = ": the file is not collated (mates do not follow each other); run `samtools collate` on it first, or match the mates by name (--bam-by-name)";

// the window after its first `cut` bytes have gone
int bam_drop_front(vs_ctx *ctx, vs_bam_stream *s, size_t cut) {
    if (int rc = s->w.keep_from(ctx, s->st, cut)) return rc;
    s->win_base += cut;
    return VS_OK;
}

int bam_too_large(vs_ctx *ctx, const vs_bam_stream *s, uint64_t bytes) {
    return vs_fail(ctx, VS_E_RANGE, "%s: a window of %llu bytes without a complete pair", s->rd.path.c_str(), (unsigned long long)bytes);
}

// the reader's next slot appended to the window: its bytes uploaded, or its BGZF members uploaded and inflated there
int bam_append(vs_ctx *ctx, vs_bam_stream *s) {
    const SlotLease lease(s->rd);
    const Slot &sl = *lease;
    if (s->w.size + sl.text > STREAM_MAX_WINDOW)
        return s->by_name ? vs_fail(ctx, VS_E_RANGE, "%s: the records that wait for their mates and the next chunk make a window of %llu bytes (the limit is %llu): "
                                                     "the mates lie too far apart to be matched by name; run `samtools collate` on the file first",
                                    s->rd.path.c_str(), (unsigned long long)(s->w.size + sl.text), (unsigned long long)STREAM_MAX_WINDOW)
                          : bam_too_large(ctx, s, s->w.size + sl.text);
    if (int rc = s->w.append(ctx, s->st, sl, s->d_stat + B_BAD_MEMBER, (uint32_t)s->w.members)) return rc;
    s->eof = sl.last;
    VS_HIP(ctx, hipStreamSynchronize(s->st));  // (the slot goes back: its bytes are on the device)
    return VS_OK;
}

// A member range: the members of the reader's slots inflated a few at a time.  Every member that starts below own_end goes
// into the window at once; behind own_end only the second record of the last owned couple is still wanted, and the members
// come one by one until it is whole.
int bam_append_ranged(vs_ctx *ctx, vs_bam_stream *s) {
    if (!s->held) {
        SlotLease lease(s->rd);
        const Slot &sl = *lease;
        if (!sl.comp || !sl.n_members) {  // (the end of the file, or bytes that are no BGZF member: pass 1 saw a whole-BGZF file)
            s->eof = sl.last;
            if (sl.len) return vs_fail(ctx, VS_E_STATE, "%s changed after its members were walked (it is not whole BGZF any more)", s->rd.path.c_str());
            return VS_OK;
        }
        if (int rc = s->w.upload_payloads(ctx, s->st, sl)) return rc == VS_E_OOM ? rc : vs_fail(ctx, VS_E_HIP, "vs_bam_stream_next: upload of a chunk");
        s->held = std::move(lease);
        s->held_at = 0;
    }
    const Slot &sl = *s->held;
    const uint32_t a = s->held_at;
    uint32_t b = a;
    uint64_t text = 0;
    for (; b < sl.n_members; b++) {
        if (b > a && s->own_end != ~0ull && s->read_pos + text >= s->own_end) break;
        text += slot_member(sl, b).isize;
    }
    int rc = s->w.size + text > STREAM_MAX_WINDOW ? bam_too_large(ctx, s, s->w.size + text)
                                                  : s->w.append_members(ctx, s->st, sl, a, b, s->d_stat + B_BAD_MEMBER, (uint32_t)s->w.members);
    if (rc == VS_OK) {
        s->held_at = b;
        s->read_pos += text;
    }
    if (b == sl.n_members) {  // (the slot is done with, whatever came of its last members)
        s->eof = sl.last;
        s->held.give_back();
    }
    return rc;
}

int bam_pass(vs_ctx *ctx, vs_bam_stream *s, uint32_t upto);

// a member range, after a scan: which of the window's records this rank owns, and the previous rank's record passed over
int bam_owned(vs_ctx *ctx, vs_bam_stream *s) {
    BamScan &sc = s->sc;
    s->own_rec = sc.n_rec;
    s->own_part = sc.n_part;
    const uint64_t lim = s->own_end == ~0ull ? ~0ull : (s->own_end > s->win_base ? s->own_end - s->win_base : 0u);
    if (lim < s->w.size && sc.n_rec) {
        VS_HIP(ctx, hipMemsetAsync(s->d_stat + B_OWN_REC, 0, sizeof(uint32_t) * 2, s->st));
        hipLaunchKernelGGL(k_bam_owned, dim3((sc.n_rec + BAM_TPB - 1u) / BAM_TPB), dim3(BAM_TPB), 0, s->st, sc.recs.as<const uint4>(), sc.part.as<const uint32_t>(),
                           sc.n_rec, sc.n_part, (uint32_t)lim, s->d_stat);
        VS_HIP(ctx, hipGetLastError());
        VS_HIP(ctx, hipMemcpyAsync(s->h_stat + B_OWN_REC, s->d_stat + B_OWN_REC, sizeof(uint32_t) * 2, hipMemcpyDeviceToHost, s->st));
        VS_HIP(ctx, hipStreamSynchronize(s->st));
        s->own_rec = std::min(s->h_stat[B_OWN_REC], sc.n_rec);
        s->own_part = std::min(s->h_stat[B_OWN_PART], sc.n_part);
    }
    if (s->skip_part && sc.n_part) {
        uint32_t first = 0;
        VS_HIP(ctx, hipMemcpyAsync(&first, sc.part.as<uint32_t>(), sizeof first, hipMemcpyDeviceToHost, s->st));
        VS_HIP(ctx, hipStreamSynchronize(s->st));
        if (first >= sc.n_rec) return vs_fail(ctx, VS_E_STATE, "%s: a record index beyond the window's records", s->rd.path.c_str());
        if (int rc = bam_pass(ctx, s, first + 1u)) return rc;
        s->part_cur = 1;
        s->skip_part = false;
    }
    return VS_OK;
}

// couples of the scanned window that can be delivered: all whole ones, or for a member range those whose first record is owned
uint64_t bam_ready(const vs_bam_stream *s) {
    const uint64_t whole = (s->sc.n_part - s->part_cur) / 2u;
    if (!s->ranged) return whole;
    const uint64_t owned = s->own_part > s->part_cur ? (s->own_part - s->part_cur + 1u) / 2u : 0u;
    return std::min(whole, owned);
}

// records [rec_cur, upto) of the scanned window have been passed: counted by class, the sums copied to the host (the copy is
// complete once the stream has been synchronised)
int bam_pass(vs_ctx *ctx, vs_bam_stream *s, uint32_t upto) {
    const uint32_t counted = s->ranged ? std::min(upto, s->own_rec) : upto;  // (a member range counts the records it owns)
    if (counted > s->rec_cur) {
        hipLaunchKernelGGL(k_bam_tally, dim3((counted - s->rec_cur + BAM_TPB - 1u) / BAM_TPB), dim3(BAM_TPB), 0, s->st, s->sc.recs.as<const uint4>(),
                           s->rec_cur, counted, s->d_stat + B_TALLY);
        VS_HIP(ctx, hipGetLastError());
        VS_HIP(ctx, hipMemcpyAsync(s->h_stat + B_TALLY, s->d_stat + B_TALLY, sizeof(uint32_t) * (B_ALL - B_TALLY), hipMemcpyDeviceToHost, s->st));
    }
    s->rec_cur = upto;
    return VS_OK;
}

// by name: the window is done.  The next one starts with its waiting records, whole and in file order, then the bytes from
// `stop` on (the record the window's end cut, or nothing)
int bam_carry_waiting(vs_ctx *ctx, vs_bam_stream *s) {
    const BamMatch &mt = s->mt;
    if (s->sc.stop > s->w.size) return vs_fail(ctx, VS_E_STATE, "%s: a record start beyond the window", s->rd.path.c_str());
    const size_t rest = s->w.size - s->sc.stop, total = (size_t)mt.wait_bytes + rest;
    uint8_t *next = nullptr;
    if (int rc = s->w.other(ctx, total, &next)) return rc;
    if (int rc = bam_carry_device(ctx, s->st, s->w.size, mt, next, mt.wait_bytes)) return rc;
    if (rest) VS_HIP(ctx, hipMemcpyAsync(next + mt.wait_bytes, s->w.data() + s->sc.stop, rest, hipMemcpyDeviceToDevice, s->st));
    s->first_record += s->sc.n_rec - s->n_carried;
    s->n_carried = mt.n_wait;
    s->waiting_max = std::max<uint64_t>(s->waiting_max, mt.n_wait);
    s->carried_bytes_max = std::max<uint64_t>(s->carried_bytes_max, mt.wait_bytes);
    s->w.flip(total);
    return VS_OK;
}

// the end of the input: what is left in the window is passed, and said if it is no whole couple
int bam_finish(vs_ctx *ctx, vs_bam_stream *s) {
    if (s->rd.err != VS_OK) return s->fail(ctx, s->rd.err, s->rd.err_msg);
    uint32_t odd = BAM_NONE;
    if (s->scanned && s->by_name) {  // (its records are counted already; what still waits has no mate in the file)
        VS_HIP(ctx, hipStreamSynchronize(s->st));
        if (s->sc.end == BAM_END_CUT) return s->fail(ctx, VS_E_ARG, rec_msg(s, s->sc.n_rec, ": truncated record (the file ends inside it)"));
        s->singletons += s->mt.n_wait;
    } else if (s->scanned) {
        if (s->sc.n_part - s->part_cur == 1u)
            VS_HIP(ctx, hipMemcpyAsync(&odd, s->sc.part.as<uint32_t>() + s->part_cur, sizeof odd, hipMemcpyDeviceToHost, s->st));
        if (int rc = bam_pass(ctx, s, s->sc.n_rec)) return s->fail(ctx, rc, vs_last_error(ctx));
        VS_HIP(ctx, hipStreamSynchronize(s->st));
        if (s->sc.end == BAM_END_CUT)
            return s->fail(ctx, VS_E_ARG, rec_msg(s, s->sc.n_rec, ": truncated record (the file ends inside it)"));
        if (odd != BAM_NONE)
            return s->fail(ctx, VS_E_ARG, rec_msg(s, odd, " has no mate behind it") + NOT_COLLATED);
    } else if (s->skip) {
        return s->fail(ctx, VS_E_STATE, s->rd.path + " ends inside its header (did it change after it was opened?)");
    }
    s->done = true;
    return VS_OK;
}

// VS_BAM_BY_NAME_KEEP, the input is at its end and its pairs are out: a singles block of up to max_reads of the records that
// still wait (mt.wlist of the last window, window order = file order), from the cursor
int bam_singles_block(vs_ctx *ctx, vs_bam_stream *s, uint64_t max_reads, vs_reads **out, uint64_t *n_slots) {
    const uint64_t n = std::min<uint64_t>(s->mt.n_wait - s->single_cur, max_reads);
    const uint32_t *list = s->mt.wlist.as<const uint32_t>() + s->single_cur;
    const VsBlockJob job = {ctx, s->st, 2u * n, &s->d_wcnt, s->d_stat + B_BLOCK, s->h_stat + B_BLOCK, VS_BLK_ST, false};
    vs_reads *r = nullptr;
    const hipError_t e1 = vs_block_bam_singles(job, BamSingles{s->w.data(), (const uint32_t *)s->sc.recs.as<uint4>(), list, s->sc.n_rec}, &r);
    if (e1 != hipSuccess) return s->fail_hip(ctx, "vs_bam_stream_next", e1);
    if (!r) {
        const uint32_t bad = s->h_stat[B_BLOCK + VS_BLK_BAD];
        if (!(bad & VS_BLK_OVER)) return s->fail(ctx, VS_E_STATE, s->rd.path + ": the waiting list of the name match names a record beyond the window's");
        return s->fail(ctx, VS_E_RANGE, rec_msg(s, fetch_u32(list + ((bad & ~VS_BLK_OVER) >> 1)), " has a sequence of more than ") + std::to_string((unsigned)VS_LEN_MASK) + " bases");
    }
    s->single_cur += (uint32_t)n;
    *out = r;
    *n_slots = n;
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_bam_header(const char *path, uint64_t *header_bytes) {
    if (!path || !header_bytes) return vs_fail(nullptr, VS_E_ARG, "vs_bam_header: bad argument");
    *header_bytes = 0;
    struct stat sb;
    if (stat(path, &sb) != 0) return vs_fail(nullptr, VS_E_ARG, "cannot open %s: %s", path, strerror(errno));
    if (!S_ISREG(sb.st_mode))  // (before it is opened: opening a FIFO would wait for its writer)
        return vs_fail(nullptr, VS_E_ARG, "%s is not a regular file: BAM is read from a regular file only (a FIFO is out of scope)", path);
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return vs_fail(nullptr, VS_E_ARG, "cannot open %s: %s", path, strerror(errno));
    struct FdGuard {
        int fd;
        ~FdGuard() { close(fd); }
    } guard = {fd};
    std::vector<uint8_t> in, text;
    size_t in_at = 0;
    bool in_eof = false;
    // header bytes needed so far, as far as the bytes at hand say: magic, l_text, text, n_ref, then per reference l_name, name, l_ref
    auto needed = [&](uint64_t *need) -> int {  // 0: *need bytes are the whole header; 1: *need bytes are needed to say more; 2: no BAM
        auto u32 = [&](uint64_t at) { return (uint64_t)bam_le32(text.data() + at); };
        if (text.size() >= 4 && memcmp(text.data(), "BAM\1", 4) != 0) return 2;
        uint64_t at = 8;
        if (text.size() < at) { *need = at; return 1; }
        at += u32(4) + 4u;
        if (text.size() < at) { *need = at; return 1; }
        const uint64_t n_ref = u32(at - 4u);
        for (uint64_t i = 0; i < n_ref; i++) {
            if (text.size() < at + 4u) { *need = at + 4u; return 1; }
            at += 4u + u32(at) + 4u;
            if (text.size() < at) { *need = at; return 1; }
        }
        *need = at;
        return 0;
    };
    for (;;) {
        uint64_t need = 0;
        const int st = needed(&need);
        if (st == 2) return vs_fail(nullptr, VS_E_ARG, "%s is not a BAM file (its first bytes do not inflate to \"BAM\\1\")", path);
        if (st == 0) {
            *header_bytes = need;
            return VS_OK;
        }
        // one more member
        vs_bgzf_member mb;
        size_t msize = 0;
        int pst;
        while ((pst = vs_bgzf_parse(in.data() + in_at, in.size() - in_at, &mb, &msize)) == 1 && !in_eof) {
            const size_t have = in.size();
            in.resize(have + (1u << 16));
            ssize_t got;
            do got = read(fd, in.data() + have, 1u << 16);
            while (got < 0 && errno == EINTR);
            if (got < 0) return vs_fail(nullptr, VS_E_ARG, "cannot read %s: %s", path, strerror(errno));
            in.resize(have + (size_t)got);
            if (got == 0) in_eof = true;
        }
        if (pst != 0) return vs_fail(nullptr, VS_E_ARG, "%s is not a BAM file (no whole BGZF member where its header goes on)", path);
        const size_t have = text.size();
        text.resize(have + mb.isize);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return vs_fail(nullptr, VS_E_OOM, "%s: zlib cannot start", path);
        zs.next_in = in.data() + in_at + mb.in_off;
        zs.avail_in = mb.in_len;
        zs.next_out = text.data() + have;
        zs.avail_out = mb.isize;
        const int rc = mb.isize ? inflate(&zs, Z_FINISH) : Z_STREAM_END;
        const bool whole = (rc == Z_STREAM_END || (rc == Z_OK && mb.isize == 0)) && zs.avail_out == 0;
        inflateEnd(&zs);
        if (!whole) return vs_fail(nullptr, VS_E_ARG, "%s: not a complete gzip stream (zlib code %d)", path, rc);
        in_at += msize;
        if (in_at == in.size() && in_eof && text.size() == have && needed(&need) != 0)
            return vs_fail(nullptr, VS_E_ARG, "%s is not a BAM file (it ends inside its header)", path);
    }
}

int vs_bam_stream_open(vs_ctx *ctx, const char *path, vs_bam_stream **out) { return vs_bam_stream_open_mode(ctx, path, VS_BAM_COLLATED, out); }

static int bam_open(vs_ctx *ctx, const char *path, int mode, const uint64_t *range, vs_bam_stream **out);

int vs_bam_stream_open_mode(vs_ctx *ctx, const char *path, int mode, vs_bam_stream **out) {
    if (!ctx || !path || !out || (mode != VS_BAM_COLLATED && mode != VS_BAM_BY_NAME && mode != VS_BAM_BY_NAME_KEEP)) return vs_fail(ctx, VS_E_ARG, "vs_bam_stream_open: bad argument");
    return bam_open(ctx, path, mode, nullptr, out);
}

int vs_bam_stream_open_range(vs_ctx *ctx, const char *path, const uint64_t range[5], vs_bam_stream **out) {
    if (!ctx || !path || !range || !out || range[3] > 1u || range[1] > range[2]) return vs_fail(ctx, VS_E_ARG, "vs_bam_stream_open_range: bad argument");
    return bam_open(ctx, path, VS_BAM_COLLATED, range, out);
}

// range: nullptr, or {file offset of the first member, bytes in front of the first record, where ownership ends (both relative
// to the first member's inflated offset; ~0: the end of the file), 1 to pass over the first participating record, that offset}
static int bam_open(vs_ctx *ctx, const char *path, int mode, const uint64_t *range, vs_bam_stream **out) {
    *out = nullptr;
    uint64_t header = 0;
    if (!range)
        if (int rc = vs_bam_header(path, &header)) return vs_fail(ctx, rc, "%s", vs_last_error(nullptr));
    VS_HIP(ctx, hipSetDevice(ctx->device));
    vs_bam_stream *s = new vs_bam_stream();
    s->device = ctx->device;
    s->skip = range ? range[1] : header;
    s->by_name = mode != VS_BAM_COLLATED;
    s->keep = mode == VS_BAM_BY_NAME_KEEP;
    if (range) {
        s->ranged = true;
        s->rd.begin = range[0];
        s->own_end = range[2];
        s->skip_part = range[3] != 0u;
        s->share_start = range[4];
    }
    if (const char *ev = getenv("VS_BAM_NAME_BITS")) s->name_bits = (uint32_t)std::min<long long>(std::max<long long>(atoll(ev), 0), 64);  // (tests: long probe chains)
    s->seg = seg_checked(0, true);
    Reader &r = s->rd;
    if (int rc = r.open_file(ctx, path)) {
        delete s;
        return rc;
    }
    hipError_t e1 = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e1 == hipSuccess) e1 = s->reserve_stat(B_ALL);
    if (e1 == hipSuccess) e1 = hipMemset(s->d_stat + B_BAD_MEMBER, 0xFF, sizeof(uint32_t));
    if (e1 != hipSuccess) {
        vs_bam_stream_close(s);
        return vs_fail(ctx, VS_E_HIP, "vs_bam_stream_open: %s", hipGetErrorString(e1));
    }
    r.th = std::thread([rp = &s->rd] { rp->run(); });
    *out = s;
    return VS_OK;
}

int vs_bam_stream_next(vs_ctx *ctx, vs_bam_stream *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs) {
    if (!ctx || !s || !out || !n_pairs) return vs_fail(ctx, VS_E_ARG, "vs_bam_stream_next: bad argument");
    *out = nullptr;
    *n_pairs = 0;
    if (s->failed != VS_OK) return s->again(ctx);
    if (s->done) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    if (!max_pairs || max_pairs > (1ull << 30)) max_pairs = 1ull << 30;
    hipStream_t st = s->st;
    BamScan &sc = s->sc;
    for (;;) {
        if (s->scanned) {
            if (s->by_name ? s->pair_cur < s->mt.n_pairs : bam_ready(s) > 0u) break;
            if (s->ranged && s->own_end != ~0ull && s->own_part <= s->part_cur &&
                (s->own_end > s->win_base ? s->own_end - s->win_base : 0u) <= (uint64_t)sc.stop) {
                // a member range: the next record starts at or behind own_end, so every owned couple is out
                if (int rc = bam_pass(ctx, s, sc.n_rec)) return s->fail(ctx, rc, vs_last_error(ctx));
                VS_HIP(ctx, hipStreamSynchronize(st));
                s->done = true;
                return VS_OK;
            }
            if (s->keep && s->eof && s->rd.err == VS_OK && sc.end != BAM_END_CUT && s->single_cur < s->mt.n_wait)
                return bam_singles_block(ctx, s, max_pairs, out, n_pairs);  // (what bam_finish would refuse comes first, there)
            if (s->eof) return bam_finish(ctx, s);
            if (s->by_name) {
                if (int rc = bam_carry_waiting(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
            } else {
                // the carry: everything from the first record not delivered
                uint32_t cut = sc.stop;
                if (s->rec_cur < sc.n_rec) {
                    VS_HIP(ctx, hipMemcpyAsync(&cut, (const uint32_t *)(sc.recs.as<uint4>() + s->rec_cur), sizeof cut, hipMemcpyDeviceToHost, st));
                    VS_HIP(ctx, hipStreamSynchronize(st));
                }
                if (cut > s->w.size) return s->fail(ctx, VS_E_STATE, s->rd.path + ": a record start beyond the window");
                if (int rc = bam_drop_front(ctx, s, cut)) return s->fail(ctx, rc, vs_last_error(ctx));
                s->first_record += s->rec_cur;
            }
            s->rec_cur = s->part_cur = s->pair_cur = s->single_cur = 0;
            s->scanned = false;
        }
        if (!s->eof) {
            if (int rc = s->ranged ? bam_append_ranged(ctx, s) : bam_append(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
            if (s->skip) {  // the header goes, whole windows of it if need be
                const size_t now = (size_t)std::min<uint64_t>(s->skip, s->w.size);
                if (int rc = bam_drop_front(ctx, s, now)) return s->fail(ctx, rc, vs_last_error(ctx));
                s->skip -= now;
                if (s->skip) {
                    if (s->eof) return bam_finish(ctx, s);
                    continue;
                }
            }
        }
        if (int rc = bam_scan_device(ctx, st, s->w.data(), s->w.size, 0, s->seg, sc, s->d_stat, s->h_stat))
            return s->fail(ctx, rc, vs_last_error(ctx));
        s->scanned = true;
        if (s->h_stat[B_BAD_MEMBER] != BAM_NONE)
            return s->fail(ctx, VS_E_ARG, s->rd.path + ": not a complete gzip stream (BGZF member " + std::to_string(s->h_stat[B_BAD_MEMBER]) +
                                                  " does not inflate to its CRC32 and size)");
        if (sc.malformed != BAM_NONE)
            return s->fail(ctx, VS_E_ARG, rec_msg(s, sc.malformed, " is malformed: its name, cigar, sequence and quality need more than its block_size"));
        if (sc.end == BAM_END_DEAD)
            return s->fail(ctx, VS_E_ARG, rec_msg(s, sc.n_rec, " is malformed: its block_size is below the 32 bytes of the fixed part"));
        if (s->ranged)
            if (int rc = bam_owned(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
        if (s->by_name) {
            s->windows++;
            s->pair_cur = 0;
            if (int rc = bam_match_device(ctx, st, s->w.data(), s->w.size, sc, s->name_bits, s->mt)) return s->fail(ctx, rc, vs_last_error(ctx));
            if (s->mt.crowded != BAM_NONE)
                return s->fail(ctx, VS_E_RANGE, rec_msg(s, s->mt.crowded, " is one of more than 64 records of one name and one end (first or second) in a window: mates "
                                                                              "are matched by name among at most 64 such records; run `samtools collate` on the file first"));
            s->rec_cur = std::min(s->n_carried, sc.n_rec);  // (the carried records were counted in their own windows)
            if (int rc = bam_pass(ctx, s, sc.n_rec)) return s->fail(ctx, rc, vs_last_error(ctx));
        }
    }
    // ---- the block of n couples from the cursor
    const uint64_t n = std::min<uint64_t>(s->by_name ? s->mt.n_pairs - s->pair_cur : bam_ready(s), max_pairs), n_ends = 2u * n;
    const uint32_t *ends = s->mt.pairs.as<const uint32_t>() + 2u * (size_t)s->pair_cur;  // by name: the pair list is (first, second), the ends as they come
    if (!s->by_name) {
        // collated: the couples checked, which record of each is which end, the cut -- three words that ride back with the builder's
        if (int rc = reserve_n<uint32_t>(ctx, s->d_ends, n_ends + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
        const hipError_t e0 = hipMemsetAsync(s->d_stat + B_BADCOUPLE, 0xFF, sizeof(uint32_t), st);
        if (e0 != hipSuccess) return s->fail_hip(ctx, "vs_bam_stream_next", e0);
        launch_ends(st, sc, s->part_cur, (uint32_t)n, s->d_ends.as<uint32_t>(), s->d_stat);
        ends = s->d_ends.as<const uint32_t>();
    }
    // (collated: the records the block passes are tallied behind it, so the last wait is here)
    const VsBlockJob job = {ctx, st, n_ends, &s->d_wcnt, s->d_stat + B_BLOCK, s->h_stat + B_BLOCK, (uint32_t)(s->by_name ? VS_BLK_ST : B_MALFORMED - B_BLOCK), !s->by_name};
    vs_reads *r = nullptr;
    hipError_t e1 = vs_block_bam(job, BamEnds{s->w.data(), (const uint32_t *)sc.recs.as<uint4>(), ends, sc.n_rec}, &r);
    if (e1 != hipSuccess) return s->fail_hip(ctx, "vs_bam_stream_next", e1);
    if (!s->by_name && s->h_stat[B_BADCOUPLE] != BAM_NONE) {
        (void)hipStreamSynchronize(st);
        vs_reads_free(ctx, r);
        const uint32_t second = fetch_u32(sc.part.as<uint32_t>() + s->part_cur + 2u * s->h_stat[B_BADCOUPLE] + 1u);
        return s->fail(ctx, VS_E_ARG, rec_msg(s, second, " is the same end (first or second) of a pair as the record it is coupled with") + NOT_COLLATED);
    }
    if (!r) {
        const uint32_t bad = s->h_stat[B_BLOCK + VS_BLK_BAD];
        if (!(bad & VS_BLK_OVER)) return s->fail(ctx, VS_E_STATE, s->rd.path + ": a pair of the name match names a record beyond the window's");
        return s->fail(ctx, VS_E_RANGE, s->rd.path + ": pair " + std::to_string(s->pairs + ((bad & ~VS_BLK_OVER) >> 1)) + " has a sequence of more than " +
                                            std::to_string((unsigned)VS_LEN_MASK) + " bases");
    }
    if (!s->by_name) {
        e1 = bam_pass(ctx, s, s->h_stat[B_CUTREC]) == VS_OK ? hipStreamSynchronize(st) : hipErrorUnknown;  // (the block is complete when it is handed out)
        if (e1 != hipSuccess) {
            vs_reads_free(ctx, r);
            return s->fail_hip(ctx, "vs_bam_stream_next", e1);
        }
    }
    if (s->by_name) s->pair_cur += (uint32_t)n;
    else s->part_cur += (uint32_t)n_ends;
    s->pairs += n;
    *out = r;
    *n_pairs = n;
    return VS_OK;
}

int vs_bam_stream_info(const vs_bam_stream *s, uint64_t info[8]) {
    if (!s || !info) return VS_E_ARG;
    const uint32_t *t = s->h_stat + B_TALLY;
    info[0] = s->pairs;
    info[1] = (uint64_t)t[0] + t[1] + t[2] + t[3] + t[4];
    info[2] = t[BAM_C_DROP900];
    info[3] = t[BAM_C_OTHER];
    info[4] = s->w.members;
    info[5] = s->rd.text_bytes;
    info[6] = s->rd.raw_bytes;
    info[7] = s->done ? 1u : 0u;
    return VS_OK;
}

int vs_bam_stream_mate_info(const vs_bam_stream *s, uint64_t info[4]) {
    if (!s || !info) return VS_E_ARG;
    info[0] = s->singletons;
    info[1] = s->waiting_max;
    info[2] = s->carried_bytes_max;
    info[3] = s->windows;
    return VS_OK;
}

void vs_bam_stream_close(vs_bam_stream *s) {
    if (!s) return;
    s->rd.shut();
    if (s->st) (void)hipStreamSynchronize(s->st);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

// ---- test aids: the chain alone -------------------------------------------------------------------------------------------
int vs_bam_scan_host(const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t *recs, uint64_t cap_recs, uint32_t *ends,
                     uint64_t cap_ends, uint64_t info[6]) {
    if ((!bytes && n) || !info || (!recs && cap_recs) || (!ends && cap_ends) || n > STREAM_MAX_WINDOW || skip > n)
        return vs_fail(nullptr, VS_E_ARG, "vs_bam_scan_host: bad argument");
    seg = seg_checked(seg);
    const uint64_t n_seg = (n + seg - 1u) / seg;
    std::vector<uint16_t> tab(n);
    std::vector<uint32_t> entry(n_seg, BAM_NONE);
    for (uint64_t s = 0; s < n_seg; s++) bam_seg_exits_serial(bytes, n, s * seg, std::min<uint64_t>(n, (s + 1u) * seg), tab.data());
    uint64_t stop = n;
    const int end = n ? bam_walk(bytes, n, tab.data(), seg, skip, entry.data(), &stop) : BAM_END_CLEAN;
    uint64_t n_rec = 0;
    uint32_t malformed = BAM_NONE, bad_couple = BAM_NONE;
    std::vector<BamRec> part;
    std::vector<uint32_t> part_idx;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (entry[s] == BAM_NONE) continue;
        uint64_t p = entry[s], at = 0;
        while (bam_seg_next(bytes, n, std::min<uint64_t>(n, (s + 1u) * seg), &p, &at)) {
            const BamRec r = bam_classify(bytes, at);
            const uint32_t cls = r.flag_cls >> 16;
            if (n_rec < cap_recs) {
                uint32_t *o = recs + 4u * n_rec;
                o[0] = r.off; o[1] = r.flag_cls; o[2] = r.l_seq; o[3] = r.seq_off;
            }
            if (cls == (uint32_t)BAM_C_MALFORMED && malformed == BAM_NONE) malformed = (uint32_t)n_rec;
            if (cls <= (uint32_t)BAM_C_SECOND) {
                part.push_back(r);
                part_idx.push_back((uint32_t)n_rec);
            }
            n_rec++;
        }
    }
    for (uint64_t c = 0; 2u * c + 1u < part.size(); c++) {
        const BamRec &a = part[2u * c], &b = part[2u * c + 1u];
        if (!bam_couple_ok(a.flag_cls, b.flag_cls) && bad_couple == BAM_NONE) bad_couple = (uint32_t)c;
        const bool a_first = (a.flag_cls >> 16) == (uint32_t)BAM_C_FIRST;
        if (2u * c < cap_ends) ends[2u * c] = part_idx[2u * c + (a_first ? 0u : 1u)];
        if (2u * c + 1u < cap_ends) ends[2u * c + 1u] = part_idx[2u * c + (a_first ? 1u : 0u)];
    }
    fill_info(info, n_rec, part.size(), (uint32_t)end, stop, malformed, bad_couple);
    return VS_OK;
}

int vs_bam_scan_text(vs_ctx *ctx, const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t *recs, uint64_t cap_recs,
                     uint32_t *ends, uint64_t cap_ends, uint64_t info[6]) {
    if (!ctx || (!bytes && n) || !info || (!recs && cap_recs) || (!ends && cap_ends) || n > STREAM_MAX_WINDOW || skip > n)
        return vs_fail(ctx, VS_E_ARG, "vs_bam_scan_text: bad argument");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    seg = seg_checked(seg);
    hipStream_t st = ctx->stream;
    VsDevBuf win, stat, d_ends;
    BamScan sc;
    uint32_t hs[B_ALL] = {0};
    VS_HIP(ctx, win.reserve(((n + 15u) & ~(uint64_t)15u) + 16u));
    VS_HIP(ctx, stat.reserve(sizeof(uint32_t) * B_ALL));
    if (n) VS_HIP(ctx, hipMemcpyAsync(win.ptr(), bytes, n, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemsetAsync(stat.ptr(), 0, sizeof(uint32_t) * B_ALL, st));
    if (int rc = bam_scan_device(ctx, st, win.as<const uint8_t>(), n, skip, seg, sc, stat.as<uint32_t>(), hs)) return rc;
    const uint32_t n_pairs = sc.n_part / 2u;
    uint32_t bad_couple = BAM_NONE;
    if (sc.n_rec && cap_recs) {
        const uint64_t m = std::min<uint64_t>(cap_recs, sc.n_rec);
        VS_HIP(ctx, hipMemcpy(recs, sc.recs.ptr(), sizeof(uint32_t) * 4u * m, hipMemcpyDeviceToHost));
    }
    if (n_pairs) {
        VS_HIP(ctx, d_ends.reserve(sizeof(uint32_t) * (2u * (size_t)n_pairs + 1u)));
        VS_HIP(ctx, hipMemsetAsync(stat.as<uint32_t>() + B_BADCOUPLE, 0xFF, sizeof(uint32_t), st));
        launch_ends(st, sc, 0, n_pairs, d_ends.as<uint32_t>(), stat.as<uint32_t>());
        VS_HIP(ctx, hipGetLastError());
        VS_HIP(ctx, hipMemcpyAsync(hs, stat.ptr(), sizeof(uint32_t) * B_ALL, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
        bad_couple = hs[B_BADCOUPLE];
        const uint64_t m = std::min<uint64_t>(cap_ends, 2u * (uint64_t)n_pairs);
        if (m) VS_HIP(ctx, hipMemcpy(ends, d_ends.ptr(), sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    }
    fill_info(info, sc.n_rec, sc.n_part, sc.end, sc.stop, sc.malformed, bad_couple);
    return VS_OK;
}

// ---- test aids: the match of one window -----------------------------------------------------------------------------------
static void mates_info(uint64_t info[3], uint64_t pairs, uint64_t waiting, uint64_t crowded) {
    info[0] = pairs;
    info[1] = waiting;
    info[2] = crowded;
}

int vs_bam_mates_host(const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t hash_bits, uint32_t *pairs, uint64_t cap_pairs,
                      uint32_t *waiting, uint64_t cap_waiting, uint64_t info[3]) {
    if ((!bytes && n) || !info || (!pairs && cap_pairs) || (!waiting && cap_waiting) || n > STREAM_MAX_WINDOW || skip > n || hash_bits > 64u)
        return vs_fail(nullptr, VS_E_ARG, "vs_bam_mates_host: bad argument");
    const uint64_t cap = n / 36u + 1u;
    std::vector<uint32_t> recs(4u * cap), ends(1);
    uint64_t sinfo[6];
    if (int rc = vs_bam_scan_host(bytes, n, skip, seg, recs.data(), cap, ends.data(), 0, sinfo)) return rc;
    std::vector<uint32_t> part;
    for (uint64_t r = 0; r < sinfo[0]; r++)
        if ((recs[4u * r + 1u] >> 16) <= (uint32_t)BAM_C_SECOND) part.push_back((uint32_t)r);
    const uint32_t np = (uint32_t)part.size(), size = bam_table_size(np);
    std::vector<uint64_t> hash(np);
    std::vector<uint32_t> table(size), head(size), slot(np), next(np), rank(np);
    BamMates m = {bytes, recs.data(), part.data(), (uint32_t)sinfo[0], np, hash.data(), table.data(), head.data(), size, slot.data(), next.data(), rank.data()};
    uint64_t minfo[4];
    bam_mates_serial(m, hash_bits, pairs, cap_pairs, waiting, cap_waiting, minfo);
    if (minfo[3]) return vs_fail(nullptr, VS_E_STATE, "vs_bam_mates_host: the name table is full");
    mates_info(info, minfo[0], minfo[1], minfo[2]);
    return VS_OK;
}

int vs_bam_mates_text(vs_ctx *ctx, const uint8_t *bytes, uint64_t n, uint64_t skip, uint32_t seg, uint32_t hash_bits, uint32_t *pairs, uint64_t cap_pairs,
                      uint32_t *waiting, uint64_t cap_waiting, uint64_t info[3]) {
    if (!ctx || (!bytes && n) || !info || (!pairs && cap_pairs) || (!waiting && cap_waiting) || n > STREAM_MAX_WINDOW || skip > n || hash_bits > 64u)
        return vs_fail(ctx, VS_E_ARG, "vs_bam_mates_text: bad argument");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    seg = seg_checked(seg);
    hipStream_t st = ctx->stream;
    VsDevBuf win, stat;
    BamScan sc;
    BamMatch mt;
    uint32_t hs[B_ALL] = {0};
    VS_HIP(ctx, win.reserve(((n + 15u) & ~(uint64_t)15u) + 16u));
    VS_HIP(ctx, stat.reserve(sizeof(uint32_t) * B_ALL));
    if (n) VS_HIP(ctx, hipMemcpyAsync(win.ptr(), bytes, n, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipMemsetAsync(stat.ptr(), 0, sizeof(uint32_t) * B_ALL, st));
    if (int rc = bam_scan_device(ctx, st, win.as<const uint8_t>(), n, skip, seg, sc, stat.as<uint32_t>(), hs)) return rc;
    if (int rc = bam_match_device(ctx, st, win.as<const uint8_t>(), n, sc, hash_bits, mt)) return rc;
    VS_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t np = std::min<uint64_t>(cap_pairs, mt.n_pairs), nw = std::min<uint64_t>(cap_waiting, mt.n_wait);
    if (np) VS_HIP(ctx, hipMemcpy(pairs, mt.pairs.ptr(), sizeof(uint32_t) * 2u * np, hipMemcpyDeviceToHost));
    if (nw) VS_HIP(ctx, hipMemcpy(waiting, mt.wlist.ptr(), sizeof(uint32_t) * nw, hipMemcpyDeviceToHost));
    mates_info(info, mt.n_pairs, mt.n_wait, mt.crowded == BAM_NONE ? ~0ull : mt.crowded);
    return VS_OK;
}

// ---- the member-sharded open, pass 1: the summary of a share ----------------------------------------------------------------
namespace {

// the tables and the lanes of one summary window
struct BamSum {
    VsDevBuf tab, cnt, lanes;
    uint32_t n_lanes = 0, seg = BAM_SEG_DEFAULT;
    uint64_t share = 0, base = 0, windows = 0;  // the share's inflated size; the position of the next window's byte 0
};

// lanes: `start` alone (rank 0: the end of the header), or every candidate [0, min(seg, share)) for start = ~0
int sum_begin(vs_ctx *ctx, hipStream_t st, BamSum &sm, uint64_t share, uint64_t start, uint32_t seg, uint64_t cap) {
    sm.seg = seg;
    sm.share = share;
    sm.base = sm.windows = 0;
    sm.n_lanes = start == ~0ull ? (uint32_t)std::min<uint64_t>(seg, share) : 1u;
    if (sm.n_lanes > cap) return vs_fail(ctx, VS_E_ARG, "the summary of a share: room for %llu entries, %u needed", (unsigned long long)cap, sm.n_lanes);
    std::vector<BamLane> lanes(sm.n_lanes);
    for (uint32_t i = 0; i < sm.n_lanes; i++) lanes[i] = BamLane{start == ~0ull ? (uint64_t)i : start, 0, BAM_LANE_LIVE, 0};
    if (int rc = reserve_n<BamLane>(ctx, sm.lanes, (size_t)sm.n_lanes + 1u)) return rc;
    if (sm.n_lanes) VS_HIP(ctx, hipMemcpyAsync(sm.lanes.ptr(), lanes.data(), sizeof(BamLane) * sm.n_lanes, hipMemcpyHostToDevice, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    return VS_OK;
}

// the window win[0, n) at position sm.base; *lim: the bytes of it that are done (the rest is the front of the next window)
int sum_window(vs_ctx *ctx, hipStream_t st, BamSum &sm, const uint8_t *win, uint64_t n, int last, uint64_t *lim) {
    *lim = bam_sum_limit(n, sm.base, sm.share, last);
    const uint64_t n_seg = (*lim + sm.seg - 1u) / sm.seg;
    if (n > STREAM_MAX_WINDOW || n_seg > 0x7FFFFFFFu) return vs_fail(ctx, VS_E_RANGE, "a BAM window of %llu bytes", (unsigned long long)n);
    if (n_seg && sm.n_lanes) {
        if (int rc = reserve_n<uint16_t>(ctx, sm.tab, *lim)) return rc;
        if (int rc = reserve_n<uint16_t>(ctx, sm.cnt, *lim)) return rc;
        hipLaunchKernelGGL(k_bam_exits_cnt, dim3((unsigned)n_seg), dim3(BAM_TPB), sizeof(uint32_t) * sm.seg, st, win, n, *lim, sm.seg, sm.tab.as<uint16_t>(),
                           sm.cnt.as<uint16_t>());
        VS_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_bam_lanes, dim3((sm.n_lanes + BAM_TPB - 1u) / BAM_TPB), dim3(BAM_TPB), 0, st, win, n, *lim, sm.tab.as<const uint16_t>(),
                           sm.cnt.as<const uint16_t>(), sm.seg, sm.base, sm.lanes.as<BamLane>(), sm.n_lanes);
        VS_HIP(ctx, hipGetLastError());
    }
    sm.base += *lim;
    sm.windows++;
    return VS_OK;
}

int sum_end(vs_ctx *ctx, hipStream_t st, BamSum &sm, uint64_t *x, uint64_t *cnt) {
    std::vector<BamLane> lanes(sm.n_lanes);
    if (sm.n_lanes) VS_HIP(ctx, hipMemcpyAsync(lanes.data(), sm.lanes.ptr(), sizeof(BamLane) * sm.n_lanes, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < sm.n_lanes; i++) {
        x[i] = bam_lane_exit(lanes[i], sm.share);
        cnt[i] = lanes[i].count;
    }
    return VS_OK;
}

// ISIZE of the member that ends at file offset `end`
int member_isize(int fd, const char *path, uint64_t end, uint32_t *isize) {
    uint8_t t[4];
    if (const char *why = end >= 4u ? pread_all(fd, t, 4, end - 4u) : "it shrank while it was read")
        return vs_fail(nullptr, VS_E_ARG, "cannot read %s: %s", path, why);
    *isize = bam_le32(t);
    return VS_OK;
}

}  // namespace

int vs_bam_share_summary_host(const uint8_t *share, uint64_t n, uint64_t share_size, uint64_t start, uint32_t seg, uint64_t chunk, uint64_t *x,
                              uint64_t *cnt, uint64_t cap, uint64_t info[2]) {
    if ((!share && n) || !info || share_size > n || n > STREAM_MAX_WINDOW || (cap && (!x || !cnt)))
        return vs_fail(nullptr, VS_E_ARG, "vs_bam_share_summary_host: bad argument");
    seg = seg_checked(seg);
    const uint32_t n_lanes = start == ~0ull ? (uint32_t)std::min<uint64_t>(seg, share_size) : 1u;
    if (n_lanes > cap) return vs_fail(nullptr, VS_E_ARG, "vs_bam_share_summary_host: room for %llu entries, %u needed", (unsigned long long)cap, n_lanes);
    const uint64_t windows = bam_share_summary_serial(share, n, share_size, start, seg, chunk, n_lanes, x, cnt);
    info[0] = n_lanes;
    info[1] = windows;
    return VS_OK;
}

int vs_bam_share_summary_text(vs_ctx *ctx, const uint8_t *share, uint64_t n, uint64_t share_size, uint64_t start, uint32_t seg, uint64_t chunk,
                              uint64_t *x, uint64_t *cnt, uint64_t cap, uint64_t info[2]) {
    if (!ctx || (!share && n) || !info || share_size > n || n > STREAM_MAX_WINDOW || (cap && (!x || !cnt)))
        return vs_fail(ctx, VS_E_ARG, "vs_bam_share_summary_text: bad argument");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    VsDevBuf dev;
    BamSum sm;
    VS_HIP(ctx, dev.reserve(((n + 15u) & ~(uint64_t)15u) + 16u));
    if (n) VS_HIP(ctx, hipMemcpyAsync(dev.ptr(), share, n, hipMemcpyHostToDevice, st));
    if (int rc = sum_begin(ctx, st, sm, share_size, start, seg_checked(seg), cap)) return rc;
    if (!chunk) chunk = n ? n : 1u;
    for (uint64_t have = std::min(n, chunk);; have = std::min(n, have + chunk)) {
        uint64_t lim = 0;
        const uint64_t base = sm.base;
        if (int rc = sum_window(ctx, st, sm, dev.as<const uint8_t>() + base, have - base, have == n, &lim)) return rc;
        if (have == n) break;
    }
    if (int rc = sum_end(ctx, st, sm, x, cnt)) return rc;
    info[0] = sm.n_lanes;
    info[1] = sm.windows;
    return VS_OK;
}

int vs_bam_share_summary(vs_ctx *ctx, const char *path, const uint64_t *offsets, uint64_t n_members, uint64_t first, uint64_t last, uint64_t start,
                         uint32_t seg, uint64_t *x, uint64_t *cnt, uint64_t cap, uint64_t info[5]) {
    if (!ctx || !path || !offsets || !info || first > last || last > n_members || (cap && (!x || !cnt)))
        return vs_fail(ctx, VS_E_ARG, "vs_bam_share_summary: bad argument");
    for (uint64_t i = first; i < n_members; i++)
        if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > 65536u)
            return vs_fail(ctx, VS_E_ARG, "vs_bam_share_summary: member %llu is no BGZF member's size", (unsigned long long)i);
    VS_HIP(ctx, hipSetDevice(ctx->device));
    seg = seg_checked(seg, true);
    struct Run {
        Reader rd;
        hipStream_t st = nullptr;
        ~Run() {
            if (st) (void)hipStreamSynchronize(st);  // (before the reader's pinned chunks go)
            rd.shut();
            if (st) (void)hipStreamDestroy(st);
        }
    } run;
    Reader &r = run.rd;
    if (int rc = r.open_file(ctx, path)) return rc;
    // the share's inflated size, and the whole members behind it that hold BAM_SUM_TAIL bytes (or the rest of the file)
    uint64_t share = 0, tail = 0, until = last;
    for (uint64_t i = first; i < last; i++) {
        uint32_t isize = 0;
        if (int rc = member_isize(r.fd, path, offsets[i + 1], &isize)) return vs_fail(ctx, rc, "%s", vs_last_error(nullptr));
        share += isize;
    }
    while (tail < (uint64_t)BAM_SUM_TAIL && until < n_members) {
        uint32_t isize = 0;
        if (int rc = member_isize(r.fd, path, offsets[until + 1], &isize)) return vs_fail(ctx, rc, "%s", vs_last_error(nullptr));
        tail += isize;
        until++;
    }
    r.begin = offsets[first];
    r.end = offsets[until];
    VS_HIP(ctx, hipStreamCreateWithFlags(&run.st, hipStreamNonBlocking));
    hipStream_t st = run.st;
    BamSum sm;
    if (int rc = sum_begin(ctx, st, sm, share, start, seg, cap)) return rc;
    DevWindow w;  // one slot + what the window before left undone
    VsDevBuf bad;
    VS_HIP(ctx, bad.reserve(sizeof(uint32_t)));
    VS_HIP(ctx, hipMemsetAsync(bad.ptr(), 0xFF, sizeof(uint32_t), st));
    uint64_t inflated = 0;
    r.th = std::thread([rp = &r] { rp->run(); });
    for (bool eof = false; !eof;) {
        const SlotLease lease(r);  // (every round ends synchronised: the slot's bytes are on the device)
        const Slot &sl = *lease;
        eof = sl.last;
        if (!sl.comp && sl.len) return vs_fail(ctx, VS_E_STATE, "%s changed after its members were walked (it is not whole BGZF any more)", path);
        if (w.size + sl.text > STREAM_MAX_WINDOW) return vs_fail(ctx, VS_E_RANGE, "a BAM window of %llu bytes", (unsigned long long)(w.size + sl.text));
        if (int rc = w.append(ctx, st, sl, bad.as<uint32_t>(), (uint32_t)(first + w.members))) return rc;
        inflated += sl.text;
        uint64_t lim = 0;
        if (int rc = sum_window(ctx, st, sm, w.data(), w.size, eof ? 1 : 0, &lim)) return rc;
        uint32_t first_bad = BAM_NONE;
        VS_HIP(ctx, hipMemcpyAsync(&first_bad, bad.ptr(), sizeof first_bad, hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
        if (first_bad != BAM_NONE)
            return vs_fail(ctx, VS_E_ARG, "%s: not a complete gzip stream (BGZF member %u does not inflate to its CRC32 and size)", path, first_bad);
        if (!eof && lim) {  // what is not done is the front of the next window
            if (int rc = w.keep_from(ctx, st, (size_t)lim)) return rc;
            VS_HIP(ctx, hipStreamSynchronize(st));
        }
    }
    if (r.err != VS_OK) return vs_fail(ctx, r.err, "%s", r.err_msg.c_str());
    if (inflated != share + tail) return vs_fail(ctx, VS_E_STATE, "%s changed after its members were walked (%llu inflated bytes where its trailers say %llu)", path,
                                                 (unsigned long long)inflated, (unsigned long long)(share + tail));
    if (int rc = sum_end(ctx, st, sm, x, cnt)) return rc;
    info[0] = sm.n_lanes;
    info[1] = share;
    info[2] = w.members;
    info[3] = r.raw_bytes;
    info[4] = sm.windows;
    return VS_OK;
}

int vs_bam_shard_plan(uint32_t world, const uint64_t *head, const uint64_t *xn, const uint64_t *xn_off, uint64_t *plan, int *reason) {
    if (!world || !head || !xn || !xn_off || !plan || !reason) return vs_fail(nullptr, VS_E_ARG, "vs_bam_shard_plan: bad argument");
    *reason = bam_shard_plan(world, head, xn, xn_off, plan);
    return VS_OK;
}

}  // extern "C"
