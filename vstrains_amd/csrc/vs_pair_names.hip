// Two FASTQ files paired by READ NAME on the device (`--check-names [--check-names-singles]`).  The plain two-file stream
// (vs_stream.hip) takes record i of either file as pair i whatever the names say: one record lost from one file -- the files
// trimmed or filtered separately -- joins two unrelated reads from there on, unnoticed.  This stream reads the same two files
// in the same forms (two Readers, two DevFiles: plain, FIFO, gzip through zlib, BGZF and plain gzip inflated on the device) and
// looks at the names (vs_pair_names_core.h has the rule, the whole-file meaning and why the result does not depend on where
// the windows are cut):
//   strict   pair p must be a pair of mates by name (il_mates of vs_mates_core.h, what --interleaved accepts side by side);
//            the first that is not stops the run, so does a complete record left over in the longer file;
//   singles  the files are in the same order but either may lack records the other has: mates are found by a hash join on
//            the names, records without a mate are dropped and counted per file.
// Per round (each window = the carried bytes, which start at a record boundary, + the slots appended since):
//   k_sl_count / k_sl_scan / k_sl_scatter   the line ends of both windows (vs_stream_lines.h); a flagged window ('\r', a byte
//                                           >= 0x80) goes through host text mode first, names are compared afterwards;
//   singles: the join of ALL complete records of both windows
//     k_pn_hash     one thread per record of both windows: key bounds at any byte alignment, the 64-bit hash;
//     k_pn_claim    the open-address table (a power of two, at most half full): claim a slot by compare-and-swap or find the
//                   key there (hash, then bytes -- the text is read-only), enter as the file's member by compare-and-swap; a
//                   taken member word is a key twice in one file (a minimum of record numbers); no lane waits for another,
//                   the probe is bounded by the table size and ends in a status word;
//     k_pn_partner  one thread per file-1 record: member[1] of its slot, decided by il_mates on the two header lines; matched
//                   records per workgroup (ballot);
//     k_sl_scan, k_pn_emit   the matched file-1 records compacted in order: rec[2p] = i, rec[2p + 1] = j; the last pair;
//     k_pn_order    one thread per pair p >= 1: rec[2p + 1] must exceed rec[2p - 1], else a minimum of p;
//   strict: k_pn_index   m[p] = il_mates(a_p, b_p) for p < min(R1, R2), the first failing p a minimum; rec is the identity.
//   ONE read-back: the pair count, the last pair, the status words.  What is decided follows on the host (pn_decide); single
//   counts are arithmetic.
// Blocks of at most max_pairs pairs are cut from rec with a cursor by the block builder (vs_block_pairs, vs_reads.hip; its source
// range-tests every rec index) -- the layout vs_pe_count takes.  When the pairs are out each
// window is cut behind its last decided record; nothing is dropped where nothing is decided.  More text goes to the file
// whose window is the smaller one (to both while both are small, to the other when one is at its end), so in-step files keep
// windows of carry + one slot.  A window beyond VS_PAIR_WINDOW bytes (default: the largest window) in a round that decided
// none of its records is refused: the files are probably not in the same order.
// Mode VS_PN_KEEP keeps the records without a mate instead of dropping them: joined and decided as singles; then, per round,
//     k_pn_mated    one thread per file-1 record: mated[mate[i]] = 1 (one byte per file-2 record, zeroed before);
//     k_pn_singles_count<Pred> / k_sl_scan / k_pn_singles_emit<Pred>   once per file, bound dec[f]: the DECIDED records in no
//                   pair compacted in file order into srec[f] (Pred: mate[i] is none / mated[j] is 0);
//   and when the round's pairs are out they are handed out as SINGLES blocks (vs_block_singles, the same builder), file 1's
//   first, then file 2's, before the windows are cut.  A record behind dec[f] waits, as it does for the pairs: it is handed
//   out once, by the round that decides it.  The other modes launch none of this.
// Inputs that are wrong end in status words and messages, never in a fault.
#include <algorithm>
#include <string>
#include <vector>

#include "vs_internal.h"
#include "vs_stream_lines.h"
#include "vs_pair_names_core.h"

#define PN_TPB SL_TPB

namespace {

// status words of a stream (file f's line scanner words at f * ST_PER_FILE)
enum {
    PS_PAIRS = 8, PS_DUP0 = 9, PS_DUP1 = 10, PS_ORDER = 11, PS_FULL = 12, PS_LAST_I = 13, PS_LAST_J = 14, PS_FIRST_BAD = 15,
    PS_BLOCK = 16,  // the VS_BLK_ST words of the block builder
    PS_ROUND = 24,  // (words below it are rewritten for every round or block)
    PS_BADM = 24,   // + f: the first BGZF member of file f the device rejected (a running index), ~0u: none
    PS_ALL = 26
};

}  // namespace

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PN_TPB) k_pn_hash(PnJoin J, uint32_t bits) {
    const uint32_t g = blockIdx.x * PN_TPB + threadIdx.x;
    if (g < J.n_all) pn_hash_at(J, g, bits);
}

__global__ void __launch_bounds__(PN_TPB) k_pn_claim(PnJoin J, uint32_t *__restrict__ st) {
    const uint32_t g = blockIdx.x * PN_TPB + threadIdx.x;
    if (g < J.n_all) pn_claim_at(J, g, &st[PS_DUP0], &st[PS_FULL]);
}

// mate[i] = the file-2 record of file-1 record i (PN_NONE: none); wg_cnt: matched records per workgroup
__global__ void __launch_bounds__(PN_TPB) k_pn_partner(PnJoin J, uint32_t *__restrict__ mate, uint32_t *__restrict__ wg_cnt) {
    __shared__ uint32_t wcnt[PN_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * PN_TPB + threadIdx.x, lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    uint32_t j = PN_NONE;
    if (i < J.f0.n_rec) mate[i] = j = pn_partner_at(J, i);
    const uint64_t b = __ballot(j != PN_NONE);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < PN_TPB / VS_WAVE; w++) t += wcnt[w];
        wg_cnt[blockIdx.x] = t;
    }
}

// wg_base: matched records in front of every workgroup, *total: all of them; rec holds two words for each of cap_pairs pairs
__global__ void __launch_bounds__(PN_TPB) k_pn_emit(const uint32_t *__restrict__ mate, const uint32_t *__restrict__ wg_base, uint32_t n_rec,
                                                    const uint32_t *total, uint32_t cap_pairs, uint32_t *__restrict__ rec,
                                                    uint32_t *__restrict__ st) {
    __shared__ uint32_t wcnt[PN_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * PN_TPB + threadIdx.x, lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    const uint32_t j = i < n_rec ? mate[i] : PN_NONE;
    const uint64_t b = __ballot(j != PN_NONE);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (j == PN_NONE) return;
    uint32_t p = wg_base[blockIdx.x] + (uint32_t)__popcll(b & (lane ? (~0ull >> (VS_WAVE - lane)) : 0ull));
    for (uint32_t w = 0; w < wave; w++) p += wcnt[w];
    if (p >= cap_pairs) return;  // (only where a key occurs twice in file 1 and both records name one of file 2: refused by the status word)
    rec[2u * p] = i;
    rec[2u * p + 1u] = j;
    if (p + 1u == *total) {
        st[PS_LAST_I] = i;
        st[PS_LAST_J] = j;
    }
}

__global__ void __launch_bounds__(PN_TPB) k_pn_order(const uint32_t *__restrict__ rec, const uint32_t *total, uint32_t cap_pairs,
                                                     uint32_t *__restrict__ st) {
    const uint32_t p = blockIdx.x * PN_TPB + threadIdx.x + 1u;
    if (p >= *total || p >= cap_pairs) return;
    if (rec[2u * p + 1u] <= rec[2u * p - 1u]) atomicMin(&st[PS_ORDER], p);
}

// VS_PN_KEEP: mated[j] = 1 for every file-2 record j that a file-1 record names (mated zeroed before; one byte per record)
__global__ void __launch_bounds__(PN_TPB) k_pn_mated(const uint32_t *__restrict__ mate, uint32_t n0, uint8_t *__restrict__ mated, uint32_t n1) {
    const uint32_t i = blockIdx.x * PN_TPB + threadIdx.x;
    if (i >= n0) return;
    const uint32_t j = mate[i];
    if (j < n1) mated[j] = 1u;
}

// VS_PN_KEEP: the records r < n (n = what the round decided of the file) with pred(r) counted per workgroup (wg_cnt, scanned
// afterwards), then srec[q] = r for the q-th of them -- a ballot, the popcount below the lane and the counts of the wavefronts
// in front, as k_pn_emit places the pairs.  One pair of kernels for both files: Pred is PnUnmated0 or PnUnmated1.
template <class Pred>
__global__ void __launch_bounds__(PN_TPB) k_pn_singles_count(Pred pred, uint32_t n, uint32_t *__restrict__ wg_cnt) {
    __shared__ uint32_t wcnt[PN_TPB / VS_WAVE];
    const uint32_t r = blockIdx.x * PN_TPB + threadIdx.x;
    const uint64_t b = __ballot(r < n && pred(r));
    if ((threadIdx.x & (VS_WAVE - 1u)) == 0u) wcnt[threadIdx.x / VS_WAVE] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < PN_TPB / VS_WAVE; w++) t += wcnt[w];
        wg_cnt[blockIdx.x] = t;
    }
}

template <class Pred>
__global__ void __launch_bounds__(PN_TPB) k_pn_singles_emit(Pred pred, const uint32_t *__restrict__ wg_base, uint32_t n, uint32_t n_singles,
                                                            uint32_t *__restrict__ srec) {
    __shared__ uint32_t wcnt[PN_TPB / VS_WAVE];
    const uint32_t r = blockIdx.x * PN_TPB + threadIdx.x, lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    const bool single = r < n && pred(r);
    const uint64_t b = __ballot(single);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!single) return;
    uint32_t q = wg_base[blockIdx.x] + (uint32_t)__popcll(b & (lane ? (~0ull >> (VS_WAVE - lane)) : 0ull));
    for (uint32_t w = 0; w < wave; w++) q += wcnt[w];
    if (q >= n_singles) return;  // (cannot be: the decided records that are in no pair are dec - pairs)
    srec[q] = r;
}

// strict: pair p = record p of either window (p < n); the first that is no pair of mates
__global__ void __launch_bounds__(PN_TPB) k_pn_index(PnWin f0, PnWin f1, uint32_t n, uint32_t *__restrict__ rec, uint32_t *__restrict__ st) {
    const uint32_t p = blockIdx.x * PN_TPB + threadIdx.x;
    if (p >= n) return;
    if (!pn_mates_at(f0, p, f1, p)) atomicMin(&st[PS_FIRST_BAD], p);
    rec[2u * p] = p;
    rec[2u * p + 1u] = p;
}

// ---- the join of one pair of windows -----------------------------------------------------------------------------------------
namespace {

struct PnDev {
    VsDevBuf hash, klen_slot, table, mate, wg;  // uint64 per record; uint32 x 2 per record; 3 T words; per file-1 record; per workgroup
    VsDevBuf mated, wg_single;                  // VS_PN_KEEP: uint8 per file-2 record; singles per workgroup -> those in front
    uint32_t n_pairs = 0, li = 0, lj = 0, dup[2] = {PN_NONE, PN_NONE}, order = PN_NONE, first_bad = PN_NONE;
};

// VS_PN_KEEP, one file of a joined round: the n_singles records r < dec with pred(r) listed in srec, in file order
template <class Pred>
int pn_compact_device(vs_ctx *ctx, hipStream_t st, const Pred &pred, uint32_t dec, uint32_t n_singles, PnDev &jd, uint32_t *srec, uint32_t *d_total) {
    if (!n_singles) return VS_OK;
    const uint32_t wgs = (dec + PN_TPB - 1u) / PN_TPB;
    if (int rc = reserve_n<uint32_t>(ctx, jd.wg_single, (size_t)wgs + 1u)) return rc;
    hipLaunchKernelGGL(k_pn_singles_count<Pred>, dim3(wgs), dim3(PN_TPB), 0, st, pred, dec, jd.wg_single.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    vs_launch_scan_u32(st, jd.wg_single.as<uint32_t>(), wgs, d_total);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pn_singles_emit<Pred>, dim3(wgs), dim3(PN_TPB), 0, st, pred, jd.wg_single.as<const uint32_t>(), dec, n_singles, srec);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// VS_PN_KEEP: the kept singles of a round that pn_join_device joined (no key twice, the pairs in order) and pn_decide decided:
// srec0 (dec[0] - n_pairs words) and srec1 (dec[1] - n_pairs words), either file's in file order.  r0 / r1: the complete
// records of the windows.  d_total: a status word for the scans' totals.  Synchronises nothing.
int pn_singles_device(vs_ctx *ctx, hipStream_t st, uint32_t r0, uint32_t r1, const uint32_t dec[2], PnDev &jd, uint32_t *srec0, uint32_t *srec1,
                      uint32_t *d_total) {
    if (dec[0] > r0 || dec[1] > r1 || jd.n_pairs > std::min(dec[0], dec[1])) return vs_fail(ctx, VS_E_STATE, "the decided records of a round do not hold its pairs");
    if (dec[0] == jd.n_pairs && dec[1] == jd.n_pairs) return VS_OK;
    if (int rc = reserve_n<uint32_t>(ctx, jd.mate, r0)) return rc;
    if (int rc = reserve_n<uint8_t>(ctx, jd.mated, r1)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, jd.wg_single, (size_t)(std::max(dec[0], dec[1]) + PN_TPB - 1u) / PN_TPB + 1u)) return rc;  // (once, for both files)
    if (r1) VS_HIP(ctx, hipMemsetAsync(jd.mated.ptr(), 0, r1, st));
    if (!std::min(r0, r1)) {  // (a window without a record: nothing was joined, mate[] was not written)
        if (r0) VS_HIP(ctx, hipMemsetAsync(jd.mate.ptr(), 0xFF, sizeof(uint32_t) * (size_t)r0, st));
    } else {
        hipLaunchKernelGGL(k_pn_mated, dim3((r0 + PN_TPB - 1u) / PN_TPB), dim3(PN_TPB), 0, st, jd.mate.as<const uint32_t>(), r0, jd.mated.as<uint8_t>(), r1);
        VS_HIP(ctx, hipGetLastError());
    }
    if (int rc = pn_compact_device(ctx, st, PnUnmated0{jd.mate.as<const uint32_t>()}, dec[0], dec[0] - jd.n_pairs, jd, srec0, d_total)) return rc;
    return pn_compact_device(ctx, st, PnUnmated1{jd.mated.as<const uint8_t>()}, dec[1], dec[1] - jd.n_pairs, jd, srec1, d_total);
}

// The pairs of the windows f0, f1 into rec (room for 2 * min(R1, R2) words): joined by name (singles), or record by record
// (strict).  table: slots (0: pn_table_size), bits: hash bits kept.  d_stat / h_stat: PS_ALL status words, [PS_PAIRS, PS_BLOCK)
// rewritten.  Synchronises the stream.
int pn_join_device(vs_ctx *ctx, hipStream_t st, const PnWin &f0, const PnWin &f1, bool singles, uint32_t table, uint32_t bits, PnDev &jd, uint32_t *rec,
                   uint32_t *d_stat, uint32_t *h_stat) {
    const uint32_t cap = std::min(f0.n_rec, f1.n_rec);
    jd.n_pairs = jd.li = jd.lj = 0;
    jd.dup[0] = jd.dup[1] = jd.order = jd.first_bad = PN_NONE;
    if (!cap) return VS_OK;
    VS_HIP(ctx, hipMemsetAsync(d_stat + PS_PAIRS, 0, sizeof(uint32_t) * (PS_BLOCK - PS_PAIRS), st));
    VS_HIP(ctx, hipMemsetAsync(d_stat + PS_DUP0, 0xFF, sizeof(uint32_t) * 3, st));  // (both duplicates, the order)
    VS_HIP(ctx, hipMemsetAsync(d_stat + PS_FIRST_BAD, 0xFF, sizeof(uint32_t), st));
    const uint32_t cap_wgs = (cap + PN_TPB - 1u) / PN_TPB;
    if (!singles) {
        hipLaunchKernelGGL(k_pn_index, dim3(cap_wgs), dim3(PN_TPB), 0, st, f0, f1, cap, rec, d_stat);
        VS_HIP(ctx, hipGetLastError());
        VS_HIP(ctx, hipMemcpyAsync(h_stat + PS_PAIRS, d_stat + PS_PAIRS, sizeof(uint32_t) * (PS_BLOCK - PS_PAIRS), hipMemcpyDeviceToHost, st));
        VS_HIP(ctx, hipStreamSynchronize(st));
        jd.first_bad = h_stat[PS_FIRST_BAD];
        jd.n_pairs = cap;
        jd.li = jd.lj = cap - 1u;
        return VS_OK;
    }
    const uint64_t n_all64 = (uint64_t)f0.n_rec + f1.n_rec;
    if (n_all64 > 0x3FFFFFFFull) return vs_fail(ctx, VS_E_RANGE, "more than 2^30 records in the two windows of a join by name");
    const uint32_t n_all = (uint32_t)n_all64, T = table ? table : pn_table_size(n_all);
    const uint32_t all_wgs = (n_all + PN_TPB - 1u) / PN_TPB, wgs0 = (f0.n_rec + PN_TPB - 1u) / PN_TPB;
    if (int rc = reserve_n<uint64_t>(ctx, jd.hash, n_all)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, jd.klen_slot, 2u * (size_t)n_all)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, jd.table, 3u * (size_t)T)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, jd.mate, f0.n_rec)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, jd.wg, (size_t)wgs0 + 1u)) return rc;
    VS_HIP(ctx, hipMemsetAsync(jd.table.ptr(), 0xFF, sizeof(uint32_t) * 3u * (size_t)T, st));
    uint32_t *tb = jd.table.as<uint32_t>();
    const PnJoin J = {f0, f1, n_all, jd.hash.as<uint64_t>(), jd.klen_slot.as<uint32_t>(), jd.klen_slot.as<uint32_t>() + n_all, T, tb, tb + T, tb + 2u * (size_t)T};
    hipLaunchKernelGGL(k_pn_hash, dim3(all_wgs), dim3(PN_TPB), 0, st, J, bits);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pn_claim, dim3(all_wgs), dim3(PN_TPB), 0, st, J, d_stat);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pn_partner, dim3(wgs0), dim3(PN_TPB), 0, st, J, jd.mate.as<uint32_t>(), jd.wg.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    vs_launch_scan_u32(st, jd.wg.as<uint32_t>(), wgs0, d_stat + PS_PAIRS);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pn_emit, dim3(wgs0), dim3(PN_TPB), 0, st, jd.mate.as<const uint32_t>(), jd.wg.as<const uint32_t>(), f0.n_rec,
                       (const uint32_t *)(d_stat + PS_PAIRS), cap, rec, d_stat);
    VS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pn_order, dim3(cap_wgs), dim3(PN_TPB), 0, st, (const uint32_t *)rec, (const uint32_t *)(d_stat + PS_PAIRS), cap, d_stat);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(h_stat + PS_PAIRS, d_stat + PS_PAIRS, sizeof(uint32_t) * (PS_BLOCK - PS_PAIRS), hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    if (h_stat[PS_FULL]) return vs_fail(ctx, VS_E_STATE, "the table of a join by name (%u slots for %u records) is full", T, n_all);
    jd.dup[0] = h_stat[PS_DUP0];
    jd.dup[1] = h_stat[PS_DUP1];
    if (jd.dup[0] != PN_NONE || jd.dup[1] != PN_NONE) return VS_OK;  // (a key twice in a window: refused, no pairs -- two records of file 1 may name one of file 2)
    if (h_stat[PS_PAIRS] > cap) return vs_fail(ctx, VS_E_STATE, "a join by name found more pairs than either window has records");
    jd.n_pairs = h_stat[PS_PAIRS];
    jd.li = h_stat[PS_LAST_I];
    jd.lj = h_stat[PS_LAST_J];
    jd.order = h_stat[PS_ORDER];
    if (jd.n_pairs && (jd.li >= f0.n_rec || jd.lj >= f1.n_rec)) return vs_fail(ctx, VS_E_STATE, "the last pair of a join by name lies outside its windows");
    return VS_OK;
}

// info of the test entries from the result of a join
void pn_join_info(uint64_t info[8], bool singles, uint32_t n_pairs, uint32_t li, uint32_t lj, const uint32_t dup[2], uint32_t order, uint32_t first_bad,
                  uint32_t r0, uint32_t r1, bool eof0, bool eof1) {
    const bool refused = dup[0] != PN_NONE || dup[1] != PN_NONE || order != PN_NONE;
    uint32_t dec[2] = {0u, 0u};
    if (!refused) {
        if (singles) pn_decide(n_pairs, li, lj, r0, r1, eof0, eof1, dec);
        else dec[0] = dec[1] = n_pairs;
    }
    info[0] = refused ? 0u : n_pairs;
    info[1] = r0;
    info[2] = r1;
    info[3] = dec[0];
    info[4] = dec[1];
    info[5] = dup[0] != PN_NONE ? dup[0] : dup[1] != PN_NONE ? (1ull << 32) | dup[1] : ~0ull;
    info[6] = order == PN_NONE || dup[0] != PN_NONE || dup[1] != PN_NONE ? ~0ull : order;  // (with a key twice the pairs are not defined, nor is their order)
    info[7] = first_bad == PN_NONE ? ~0ull : first_bad;
}

}  // namespace

// ---- the stream ------------------------------------------------------------------------------------------------------------
struct vs_fastq_pn : StreamState {  // (PS_ALL status words)
    int device = 0;
    hipStream_t st = nullptr;
    Reader rd[2];
    DevFile df[2];
    PnDev jd;
    VsDevBuf rec;            // uint32: rec[2p], rec[2p + 1] = the records of the round's p-th pair
    bool joined = false;     // jd and rec describe the windows
    uint32_t pair_cur = 0;   // the first pair of the round not yet delivered
    uint32_t dec[2] = {0, 0};  // records of either window the round decided
    bool singles_mode = false;
    bool keep = false;             // VS_PN_KEEP: the decided records without a mate are handed out as singles blocks
    VsDevBuf srec[2];              // VS_PN_KEEP: srec[f][q] = the q-th kept single of file f's window, in file order
    uint32_t n_single[2] = {0, 0}, single_cur[2] = {0, 0};  // ... how many the round has, the first not yet delivered
    size_t window_limit = STREAM_MAX_WINDOW;
    uint32_t name_bits = 64;  // bits of the name hash kept (VS_PAIR_NAME_BITS: tests)
    VsDevBuf d_wcnt;
    uint64_t pairs = 0, singles[2] = {0, 0}, records[2] = {0, 0}, windows = 0, max_window = 0;
    uint32_t flags_seen = 0;
};

namespace {

PnWin pn_win(const DevFile &d) { return PnWin{d.w.data(), d.ends.as<const uint32_t>(), d.n_nl, (uint32_t)d.w.size, (uint32_t)d.records}; }

// count + scan of both windows: line ends counted, flags, records (synchronises the stream)
int pn_scan(vs_ctx *ctx, vs_fastq_pn *s) {
    VS_HIP(ctx, hipMemsetAsync(s->d_stat, 0, sizeof(uint32_t) * 2u * ST_PER_FILE, s->st));
    for (int f = 0; f < 2; f++) {
        DevFile &d = s->df[f];
        if (int rc = reserve_n<uint32_t>(ctx, d.wg, sl_workgroups(d.w.size) + 1u)) return rc;
        vs_launch_sl_count(s->st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), s->d_stat + f * ST_PER_FILE);
    }
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(s->h_stat, s->d_stat, sizeof(uint32_t) * PS_ALL, hipMemcpyDeviceToHost, s->st));
    VS_HIP(ctx, hipStreamSynchronize(s->st));
    for (int f = 0; f < 2; f++) {
        s->df[f].take_status(s->h_stat + f * ST_PER_FILE);
        s->flags_seen |= s->df[f].flags;
    }
    return VS_OK;
}

// the header line of record r of window f, for a message (at most 200 bytes of it)
std::string pn_header_line(vs_fastq_pn *s, int f, uint32_t r) {
    const DevFile &d = s->df[f];
    uint32_t e[2] = {0, 0};
    const uint32_t *ends = d.ends.as<const uint32_t>();
    if (4ull * r >= d.n_nl) return "?";
    if (r && hipMemcpy(&e[0], ends + 4u * (size_t)r - 1u, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return "?";
    if (hipMemcpy(&e[1], ends + 4u * (size_t)r, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return "?";
    const size_t a = r ? (size_t)e[0] + 1u : 0u, b = e[1];
    if (a > b || b > d.w.size) return "?";
    std::string line(std::min<size_t>(b - a, 200u), '\0');
    if (!line.empty() && hipMemcpy(&line[0], d.w.data() + a, line.size(), hipMemcpyDeviceToHost) != hipSuccess) return "?";
    return line;
}

// the key of that line, for a message
std::string pn_key_of(const std::string &line, int f) { return line.substr(0, pn_key_len((const uint8_t *)line.data(), (uint32_t)line.size(), (uint32_t)f)); }

// the end of the input: a reader's failure, if it had one (in file order)
int pn_finish(vs_ctx *ctx, vs_fastq_pn *s) {
    for (int f = 0; f < 2; f++)
        if (s->rd[f].err != VS_OK) return s->fail(ctx, s->rd[f].err, s->rd[f].err_msg);
    s->done = true;
    return VS_OK;
}

// The next round: the decided records of the last one cut off, more text appended, the line ends found, the records joined.
// *end: nothing more comes (the stream is done or has failed; the code is returned).
int pn_next_round(vs_ctx *ctx, vs_fastq_pn *s, bool *end) {
    hipStream_t st = s->st;
    *end = true;
    if (s->joined) {
        if (s->df[0].eof && s->df[1].eof) return pn_finish(ctx, s);  // (everything was decided)
        for (int f = 0; f < 2; f++) {
            DevFile &d = s->df[f];
            if (!s->dec[f]) continue;  // (nothing decided: nothing dropped)
            uint32_t at = 0;  // one past the line end that closes the last decided record
            const size_t line = 4u * (size_t)s->dec[f] - 1u;
            size_t cut = d.w.size;  // (a last line without a line end, at the end of the file)
            if (line < d.n_nl) {
                VS_HIP(ctx, hipMemcpyAsync(&at, d.ends.as<uint32_t>() + line, sizeof at, hipMemcpyDeviceToHost, st));
                VS_HIP(ctx, hipStreamSynchronize(st));
                cut = (size_t)at + 1u;
            }
            if (cut > d.w.size) return s->fail(ctx, VS_E_STATE, s->rd[f].path + ": a line end beyond the window");
            if (int rc = drop_front(ctx, st, d, cut, s->dec[f])) return s->fail(ctx, rc, vs_last_error(ctx));
        }
        s->joined = false;
        s->pair_cur = 0;
        s->dec[0] = s->dec[1] = 0;
        s->n_single[0] = s->n_single[1] = s->single_cur[0] = s->single_cur[1] = 0;
    }
    {
        // more text: for the smaller window, for both while both are below half a chunk, for the other when one is at its end
        SlotLease taken[2];  // (go back once the stream is synchronised: the uploads are done)
        bool fresh[2] = {false, false};
        for (int f = 0; f < 2; f++) {
            DevFile &d = s->df[f], &o = s->df[f ^ 1];
            if (d.eof || !(o.eof || d.w.size <= o.w.size || d.w.size < s->rd[f].chunk / 2u)) continue;
            if (int rc = append_chunk(ctx, st, d, s->rd[f], taken[f], s->d_stat + PS_BADM + f)) return s->fail(ctx, rc, vs_last_error(ctx));
            fresh[f] = true;
        }
        if (int rc = pn_scan(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
        for (int f = 0; f < 2; f++)
            if (fresh[f] && taken[f]) (void)member_failed(s->df[f], s->rd[f], *taken[f], s->h_stat[PS_BADM + f]);
        for (int f = 0; f < 2; f++) taken[f].give_back();
        bool again = false;
        for (int f = 0; f < 2; f++) {
            DevFile &d = s->df[f];
            if (d.err == VS_OK && fresh[f] && d.flags && d.validated < d.w.size)  // (text that arrived with this slot: host text mode)
                if (translate_window(ctx, d, s->rd[f].path) == VS_OK) again = true;
        }
        if (again)
            if (int rc = pn_scan(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
    }
    for (int f = 0; f < 2; f++) {
        DevFile &d = s->df[f];
        Reader &r = s->rd[f];
        if (d.err != VS_OK) return s->fail(ctx, r.err != VS_OK ? r.err : d.err, r.err != VS_OK ? r.err_msg : d.err_msg);
        if (d.records > 0x3FFFFFFFull) return s->fail(ctx, VS_E_RANGE, r.path + ": more than 2^30 records in one window");
        if (int rc = reserve_n<uint32_t>(ctx, d.ends, (size_t)d.n_nl + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
        vs_launch_sl_scatter(st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), d.ends.as<uint32_t>());
        s->max_window = std::max<uint64_t>(s->max_window, d.w.size);
    }
    VS_HIP(ctx, hipGetLastError());
    s->windows++;
    const PnWin f0 = pn_win(s->df[0]), f1 = pn_win(s->df[1]);
    const bool eof[2] = {s->df[0].eof, s->df[1].eof};
    if (int rc = reserve_n<uint32_t>(ctx, s->rec, 2u * (size_t)std::min(f0.n_rec, f1.n_rec) + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
    if (int rc = pn_join_device(ctx, st, f0, f1, s->singles_mode, 0u, s->name_bits, s->jd, s->rec.as<uint32_t>(), s->d_stat, s->h_stat)) return s->fail(ctx, rc, vs_last_error(ctx));
    s->joined = true;
    const PnDev &j = s->jd;
    const std::string &p0 = s->rd[0].path, &p1 = s->rd[1].path;
    if (!s->singles_mode) {
        if (j.first_bad != PN_NONE) {
            const uint32_t p = j.first_bad;
            return s->fail(ctx, VS_E_ARG,
                           p0 + " / " + p1 + ": pair " + std::to_string(s->df[0].first_record + p) + " is no pair of mates by name: \"" + pn_header_line(s, 0, p) + "\" against \"" +
                               pn_header_line(s, 1, p) + "\".  --check-names takes record i of either file as pair i and stops where their names differ (a record "
                                                         "lost from one file?); to drop and count the records without a mate, add --check-names-singles");
        }
        s->dec[0] = s->dec[1] = j.n_pairs;
        const int longer = (eof[1] && f0.n_rec > f1.n_rec) ? 0 : (eof[0] && f1.n_rec > f0.n_rec) ? 1 : -1;  // (the other file has ended, all of it is here)
        if (longer >= 0) {
            const int f = longer;
            const uint32_t r = std::min(f0.n_rec, f1.n_rec);
            return s->fail(ctx, VS_E_ARG,
                           p0 + " / " + p1 + ": pair " + std::to_string(s->df[f].first_record + r) + " has no record in " + s->rd[f ^ 1].path + ", which ends there: \"" +
                               pn_header_line(s, f, r) + "\" of " + s->rd[f].path + " against end of file.  --check-names stops at a record left over in the longer "
                                                                                   "file; to drop and count the records without a mate, add --check-names-singles");
        }
    } else {
        for (int f = 0; f < 2; f++)
            if (j.dup[f] != PN_NONE) {
                const std::string line = pn_header_line(s, f, j.dup[f]);
                return s->fail(ctx, VS_E_ARG,
                               "name " + pn_key_of(line, f) + " occurs twice in " + s->rd[f].path + " (record " + std::to_string(s->df[f].first_record + j.dup[f]) + ", \"" + line +
                                   "\", is the first of them): --check-names-singles joins the two files by read name, and within a file a name stands for one record");
            }
        if (j.order != PN_NONE) {
            uint32_t q[4] = {0, 0, 0, 0};  // the pair before it and the pair itself
            VS_HIP(ctx, hipMemcpy(q, s->rec.as<uint32_t>() + 2u * (size_t)j.order - 2u, sizeof q, hipMemcpyDeviceToHost));
            return s->fail(ctx, VS_E_ARG,
                           p0 + " record " + std::to_string(s->df[0].first_record + q[2]) + " and " + p1 + " record " + std::to_string(s->df[1].first_record + q[3]) + " (\"" +
                               pn_header_line(s, 0, q[2]) + "\") are mates but lie behind " + p0 + " record " + std::to_string(s->df[0].first_record + q[0]) + " and in front of its mate, " +
                               p1 + " record " + std::to_string(s->df[1].first_record + q[1]) + ": --check-names-singles needs both files in the same order");
        }
        pn_decide(j.n_pairs, j.li, j.lj, f0.n_rec, f1.n_rec, eof[0], eof[1], s->dec);
        for (int f = 0; f < 2; f++) {
            const DevFile &d = s->df[f];
            if (!s->dec[f] && d.w.size > s->window_limit && !(eof[0] && eof[1]))
                return s->fail(ctx, VS_E_RANGE,
                               s->rd[f].path + ": " + std::to_string(d.records) + " records of this file wait without a mate in a window of " + std::to_string(d.w.size) +
                                   " bytes (limit " + std::to_string(s->window_limit) + "; " + std::to_string(s->df[f ^ 1].records) + " records of " + s->rd[f ^ 1].path +
                                   " wait too): the two files are probably not in the same order");
        }
    }
    if (s->dec[0] > f0.n_rec || s->dec[1] > f1.n_rec || j.n_pairs > std::min(s->dec[0], s->dec[1]))
        return s->fail(ctx, VS_E_STATE, "the decided records of a round do not hold its pairs");
    for (int f = 0; f < 2; f++) {
        s->records[f] += s->dec[f];
        s->singles[f] += s->dec[f] - j.n_pairs;
    }
    if (s->keep) {
        for (int f = 0; f < 2; f++)
            if (int rc = reserve_n<uint32_t>(ctx, s->srec[f], (size_t)(s->dec[f] - j.n_pairs) + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
        if (int rc = pn_singles_device(ctx, st, f0.n_rec, f1.n_rec, s->dec, s->jd, s->srec[0].as<uint32_t>(), s->srec[1].as<uint32_t>(), s->d_stat + PS_BLOCK + VS_BLK_WORDS))
            return s->fail(ctx, rc, vs_last_error(ctx));
        for (int f = 0; f < 2; f++) s->n_single[f] = s->dec[f] - j.n_pairs;
    }
    *end = false;
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_fastq_pn_open(vs_ctx *ctx, const char *fwd_path, const char *rve_path, int mode, vs_fastq_pn **out) {
    if (!ctx || !fwd_path || !rve_path || !out || (mode != VS_PN_STRICT && mode != VS_PN_SINGLES && mode != VS_PN_KEEP)) return vs_fail(ctx, VS_E_ARG, "vs_fastq_pn_open: bad argument");
    *out = nullptr;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    vs_fastq_pn *s = new vs_fastq_pn();
    s->device = ctx->device;
    s->singles_mode = mode != VS_PN_STRICT;
    s->keep = mode == VS_PN_KEEP;
    if (const char *ev = getenv("VS_PAIR_WINDOW")) s->window_limit = (size_t)std::min<long long>(std::max<long long>(1, atoll(ev)), (long long)STREAM_MAX_WINDOW);  // (tests)
    if (const char *ev = getenv("VS_PAIR_NAME_BITS")) s->name_bits = (uint32_t)std::min<long long>(std::max<long long>(1, atoll(ev)), 64);  // (tests: shared probe chains)
    const char *paths[2] = {fwd_path, rve_path};
    for (int f = 0; f < 2; f++) {
        Reader &r = s->rd[f];
        fastq_switches(r, false, s->df[f].w.gz.text_cap);
        if (int rc = r.open_file(ctx, paths[f])) {
            for (int g = 0; g < f; g++) close(s->rd[g].fd);
            for (int g = 0; g < 2; g++) s->rd[g].fd = -1;
            delete s;
            return rc;
        }
    }
    hipError_t e1 = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e1 == hipSuccess) e1 = s->reserve_stat(PS_ALL);
    if (e1 == hipSuccess) e1 = hipMemset(s->d_stat + PS_BADM, 0xFF, sizeof(uint32_t) * 2);
    if (e1 != hipSuccess) {
        vs_fastq_pn_close(s);
        return vs_fail(ctx, VS_E_HIP, "vs_fastq_pn_open: %s", hipGetErrorString(e1));
    }
    for (int f = 0; f < 2; f++) s->rd[f].th = std::thread([r = &s->rd[f]] { r->run(); });
    *out = s;
    return VS_OK;
}

int vs_fastq_pn_next(vs_ctx *ctx, vs_fastq_pn *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs) {
    if (!ctx || !s || !out || !n_pairs) return vs_fail(ctx, VS_E_ARG, "vs_fastq_pn_next: bad argument");
    *out = nullptr;
    *n_pairs = 0;
    if (s->failed != VS_OK) return s->again(ctx);
    if (s->done) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    if (!max_pairs || max_pairs > (1ull << 30)) max_pairs = 1ull << 30;
    while (!s->joined || (s->pair_cur >= s->jd.n_pairs && s->single_cur[0] >= s->n_single[0] && s->single_cur[1] >= s->n_single[1])) {
        bool end = false;
        const int rc = pn_next_round(ctx, s, &end);
        if (end) return rc;
    }
    // ---- the block of n pairs from the cursor -- or, VS_PN_KEEP and the round's pairs out, a singles block of n kept records of
    // file 1 or, once those are out, of file 2 (file f): rec[i] = the record of the block's i-th end / read
    const bool single = s->pair_cur >= s->jd.n_pairs;
    const int f = s->single_cur[0] < s->n_single[0] ? 0 : 1;
    const uint64_t n = std::min<uint64_t>(single ? s->n_single[f] - s->single_cur[f] : s->jd.n_pairs - s->pair_cur, max_pairs);
    const uint32_t *rec = single ? s->srec[f].as<const uint32_t>() + s->single_cur[f] : s->rec.as<const uint32_t>() + 2u * (size_t)s->pair_cur;
    const PnWin f0 = pn_win(s->df[0]), f1 = pn_win(s->df[1]);
    const SlWin w[2] = {{f0.txt, f0.ends, f0.n_nl, f0.size}, {f1.txt, f1.ends, f1.n_nl, f1.size}};
    const VsBlockJob job = {ctx, s->st, 2u * n, &s->d_wcnt, s->d_stat + PS_BLOCK, s->h_stat + PS_BLOCK, VS_BLK_ST, false};
    vs_reads *r = nullptr;
    const hipError_t e1 = single ? vs_block_singles(job, w[f], rec, 0u, &r) : vs_block_pairs(job, w[0], f0.n_rec, w[1], f1.n_rec, rec, &r);
    if (e1 != hipSuccess) return s->fail_hip(ctx, "vs_fastq_pn_next", e1);
    if (!r) {
        const uint32_t bad = s->h_stat[PS_BLOCK + VS_BLK_BAD], e = bad & ~VS_BLK_OVER;
        if (!(bad & VS_BLK_OVER)) return s->fail(ctx, VS_E_STATE, "vs_fastq_pn_next: a pair names a record outside its window");
        const int g = single ? f : (int)(e & 1u);
        return s->fail(ctx, VS_E_RANGE, too_long_line(s->rd[g].path, s->df[g].first_record + fetch_u32(rec + (single ? e >> 1 : e))));
    }
    if (single) s->single_cur[f] += (uint32_t)n;
    else s->pair_cur += (uint32_t)n, s->pairs += n;
    *out = r;
    *n_pairs = n;
    return VS_OK;
}

int vs_fastq_pn_info(const vs_fastq_pn *s, uint64_t info[10]) {
    if (!s || !info) return VS_E_ARG;
    info[0] = s->pairs;
    info[1] = s->singles[0];
    info[2] = s->singles[1];
    info[3] = s->records[0];
    info[4] = s->records[1];
    info[5] = s->windows;
    info[6] = s->max_window;
    info[7] = s->rd[0].text_bytes + s->rd[1].text_bytes + s->df[0].w.gz.text + s->df[1].w.gz.text;
    info[8] = s->rd[0].raw_bytes + s->rd[1].raw_bytes;
    info[9] = (uint64_t)s->flags_seen | (s->rd[0].gzip ? 4u : 0u) | (s->rd[1].gzip ? 8u : 0u) | (s->done ? 16u : 0u);
    return VS_OK;
}

void vs_fastq_pn_close(vs_fastq_pn *s) {
    if (!s) return;
    for (Reader &r : s->rd) r.shut();
    if (s->st) (void)hipStreamSynchronize(s->st);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

// ---- test aids: the join of one pair of windows ----------------------------------------------------------------------------
namespace {

// line ends and complete records of host text
static void pn_host_lines(const uint8_t *text, uint64_t n, int eof, std::vector<uint32_t> &ends, uint32_t *n_rec) {
    for (uint64_t i = 0; i < n; i++)
        if (text[i] == '\n') ends.push_back((uint32_t)i);
    const uint64_t lines = ends.size() + ((eof && n && text[n - 1u] != '\n') ? 1u : 0u);
    *n_rec = (uint32_t)(lines / 4u);
}

static bool pn_table_ok(uint32_t table) { return table == 0u || (table >= 2u && table <= (1u << 30) && (table & (table - 1u)) == 0u); }

}  // namespace

// vs_fastq_join_host, and with `sing` vs_fastq_join_singles_host: the kept singles of either window too (info has 10 words then)
struct PnSinglesOut {
    uint32_t *list[2];
    uint64_t cap[2];
};

static int pn_join_host_entry(const char *who, const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                              uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, const PnSinglesOut *sing, uint64_t *info) {
    if ((!text0 && n0) || (!text1 && n1) || !info || (!pairs && cap_pairs) || n0 > STREAM_MAX_WINDOW || n1 > STREAM_MAX_WINDOW || !pn_table_ok(table) ||
        (sing ? (mode != VS_PN_SINGLES && mode != VS_PN_KEEP) || (!sing->list[0] && sing->cap[0]) || (!sing->list[1] && sing->cap[1])
              : (mode != VS_PN_STRICT && mode != VS_PN_SINGLES)))
        return vs_fail(nullptr, VS_E_ARG, "%s: bad argument", who);
    std::vector<uint32_t> e0, e1;
    uint32_t r0 = 0, r1 = 0;
    pn_host_lines(text0, n0, eof0, e0, &r0);
    pn_host_lines(text1, n1, eof1, e1, &r1);
    const PnWin f0 = {text0, e0.data(), (uint32_t)e0.size(), (uint32_t)n0, r0}, f1 = {text1, e1.data(), (uint32_t)e1.size(), (uint32_t)n1, r1};
    const uint32_t cap = std::min(r0, r1), n_all = r0 + r1;
    std::vector<uint32_t> rec(2u * (size_t)cap + 1u);
    uint32_t res[5] = {0u, PN_NONE, PN_NONE, PN_NONE, 0u}, first_bad = PN_NONE;
    std::vector<uint32_t> mate(r0 ? r0 : 1u, PN_NONE);
    if (mode == VS_PN_STRICT) {
        for (uint32_t p = 0; p < cap; p++) {
            if (first_bad == PN_NONE && !pn_mates_at(f0, p, f1, p)) first_bad = p;
            rec[2u * p] = rec[2u * p + 1u] = p;
        }
        res[0] = cap;
    } else {
        const uint32_t T = table ? table : pn_table_size(n_all);
        std::vector<uint64_t> hash(n_all ? n_all : 1u);
        std::vector<uint32_t> klen_slot(2u * (size_t)n_all + 1u), tb(3u * (size_t)T);
        const PnJoin J = {f0, f1, n_all, hash.data(), klen_slot.data(), klen_slot.data() + n_all, T, tb.data(), tb.data() + T, tb.data() + 2u * (size_t)T};
        pn_join_host(J, name_bits ? name_bits : 64u, rec.data(), res);
        if (res[4]) return vs_fail(nullptr, VS_E_STATE, "the table of a join by name (%u slots for %u records) is full", T, n_all);
        if (sing)
            for (uint32_t i = 0; i < r0; i++) mate[i] = pn_partner_at(J, i);  // (as k_pn_partner leaves it)
    }
    const uint32_t P = std::min(res[0], cap);
    pn_join_info(info, mode != VS_PN_STRICT, P, P ? rec[2u * P - 2u] : 0u, P ? rec[2u * P - 1u] : 0u, &res[1], res[3], first_bad, r0, r1, eof0 != 0, eof1 != 0);
    const uint64_t np = std::min<uint64_t>(cap_pairs, info[0]);
    if (np) memcpy(pairs, rec.data(), sizeof(uint32_t) * 2u * np);
    if (sing) {  // (a refused round decides nothing: info[3] = info[4] = 0, no singles)
        std::vector<uint8_t> mated(r1 ? r1 : 1u);
        pn_mated_host(mate.data(), r0, mated.data(), r1);
        info[8] = pn_singles_host(PnUnmated0{mate.data()}, (uint32_t)info[3], sing->list[0], sing->cap[0]);
        info[9] = pn_singles_host(PnUnmated1{mated.data()}, (uint32_t)info[4], sing->list[1], sing->cap[1]);
    }
    return VS_OK;
}

int vs_fastq_join_host(const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table, uint32_t name_bits,
                       uint32_t *pairs, uint64_t cap_pairs, uint64_t info[8]) {
    return pn_join_host_entry("vs_fastq_join_host", text0, n0, text1, n1, eof0, eof1, mode, table, name_bits, pairs, cap_pairs, nullptr, info);
}

int vs_fastq_join_singles_host(const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                               uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, uint32_t *singles0, uint64_t cap_singles0, uint32_t *singles1,
                               uint64_t cap_singles1, uint64_t info[10]) {
    const PnSinglesOut sing = {{singles0, singles1}, {cap_singles0, cap_singles1}};
    return pn_join_host_entry("vs_fastq_join_singles_host", text0, n0, text1, n1, eof0, eof1, mode, table, name_bits, pairs, cap_pairs, &sing, info);
}

static int pn_join_text_entry(const char *who, vs_ctx *ctx, const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode,
                              uint32_t table, uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, const PnSinglesOut *sing, uint32_t guard, uint64_t *info) {
    if (!ctx || (!text0 && n0) || (!text1 && n1) || !info || (!pairs && cap_pairs) || n0 > STREAM_MAX_WINDOW || n1 > STREAM_MAX_WINDOW || !pn_table_ok(table) ||
        (sing ? (mode != VS_PN_SINGLES && mode != VS_PN_KEEP) || (!sing->list[0] && sing->cap[0]) || (!sing->list[1] && sing->cap[1])
              : (mode != VS_PN_STRICT && mode != VS_PN_SINGLES)) ||
        guard > (1u << 20))
        return vs_fail(ctx, VS_E_ARG, "%s: bad argument", who);
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t SENTINEL = 0xA5C3F00Du;
    const uint8_t *text[2] = {text0, text1};
    const uint64_t n[2] = {n0, n1};
    const int eof[2] = {eof0, eof1};
    VsDevBuf txt[2], wg[2], ends[2], stat, rec;
    PnDev jd;
    PnWin w[2];
    uint32_t hs[PS_ALL] = {0};
    VS_HIP(ctx, stat.reserve(sizeof(uint32_t) * PS_ALL));
    VS_HIP(ctx, hipMemsetAsync(stat.ptr(), 0, sizeof(uint32_t) * PS_ALL, st));
    for (int f = 0; f < 2; f++) {
        const uint64_t wgs = sl_workgroups(n[f]);
        VS_HIP(ctx, txt[f].reserve(DevWindow::padded(n[f])));
        VS_HIP(ctx, wg[f].reserve(sizeof(uint32_t) * (wgs + 1u)));
        if (n[f]) VS_HIP(ctx, hipMemcpyAsync(txt[f].ptr(), text[f], n[f], hipMemcpyHostToDevice, st));
        vs_launch_sl_count(st, txt[f].as<const uint8_t>(), n[f], wg[f].as<uint32_t>(), stat.as<uint32_t>() + f * ST_PER_FILE);
        VS_HIP(ctx, hipGetLastError());
    }
    VS_HIP(ctx, hipMemcpyAsync(hs, stat.ptr(), sizeof(uint32_t) * 2u * ST_PER_FILE, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    for (int f = 0; f < 2; f++) {
        const uint32_t *h = hs + f * ST_PER_FILE;
        const uint64_t lines = (uint64_t)h[ST_NL] + ((eof[f] && n[f] && h[ST_LAST] != '\n') ? 1u : 0u);
        VS_HIP(ctx, ends[f].reserve(sizeof(uint32_t) * ((size_t)h[ST_NL] + 1u)));
        vs_launch_sl_scatter(st, txt[f].as<const uint8_t>(), n[f], wg[f].as<const uint32_t>(), ends[f].as<uint32_t>());
        VS_HIP(ctx, hipGetLastError());
        w[f] = PnWin{txt[f].as<const uint8_t>(), ends[f].as<const uint32_t>(), h[ST_NL], (uint32_t)n[f], (uint32_t)(lines / 4u)};
    }
    // the pair list, at its full capacity, between two rows of `guard` sentinel words
    const uint32_t cap = std::min(w[0].n_rec, w[1].n_rec);
    const size_t body = 2u * (size_t)cap, all = body + 2u * (size_t)guard;
    std::vector<uint32_t> h(all ? all : 1u, SENTINEL);
    VS_HIP(ctx, rec.reserve(sizeof(uint32_t) * (all ? all : 1u)));
    if (all) VS_HIP(ctx, hipMemcpyAsync(rec.ptr(), h.data(), sizeof(uint32_t) * all, hipMemcpyHostToDevice, st));
    if (int rc = pn_join_device(ctx, st, w[0], w[1], mode != VS_PN_STRICT, table, name_bits ? name_bits : 64u, jd, rec.as<uint32_t>() + guard, stat.as<uint32_t>(), hs)) return rc;
    if (all) VS_HIP(ctx, hipMemcpyAsync(h.data(), rec.ptr(), sizeof(uint32_t) * all, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    for (uint32_t g = 0; g < guard; g++)
        if (h[g] != SENTINEL || h[guard + body + g] != SENTINEL) return vs_fail(ctx, VS_E_STATE, "vs_fastq_join_text: a kernel wrote outside the pair list");
    const bool twice = jd.dup[0] != PN_NONE || jd.dup[1] != PN_NONE;  // (then the list holds whatever matched, and nothing of it is given)
    for (size_t k = 0; !twice && k < 2u * (size_t)jd.n_pairs; k++)
        if (h[guard + k] == SENTINEL) return vs_fail(ctx, VS_E_STATE, "vs_fastq_join_text: a word of the pair list was not written");
    for (size_t k = 2u * (size_t)jd.n_pairs; !twice && k < body; k++)
        if (h[guard + k] != SENTINEL) return vs_fail(ctx, VS_E_STATE, "vs_fastq_join_text: a word behind the pair list was written");
    pn_join_info(info, mode != VS_PN_STRICT, jd.n_pairs, jd.li, jd.lj, jd.dup, jd.order, jd.first_bad, w[0].n_rec, w[1].n_rec, eof0 != 0, eof1 != 0);
    const uint64_t np = std::min<uint64_t>(cap_pairs, info[0]);
    if (np) memcpy(pairs, h.data() + guard, sizeof(uint32_t) * 2u * np);
    if (!sing) return VS_OK;
    // the kept singles of what the round decides: either list at its exact size between two rows of `guard` sentinel words
    const uint32_t dec[2] = {(uint32_t)info[3], (uint32_t)info[4]};
    const uint32_t P = (uint32_t)info[0];  // (0 where the round is refused: then nothing is decided either)
    if (dec[0] < P || dec[1] < P) return vs_fail(ctx, VS_E_STATE, "%s: the decided records of the round do not hold its pairs", who);
    const size_t ns[2] = {(size_t)(dec[0] - P), (size_t)(dec[1] - P)};
    VsDevBuf srec[2];
    std::vector<uint32_t> hl[2];
    for (int f = 0; f < 2; f++) {
        hl[f].assign(ns[f] + 2u * (size_t)guard + 1u, SENTINEL);
        VS_HIP(ctx, srec[f].reserve(sizeof(uint32_t) * hl[f].size()));
        VS_HIP(ctx, hipMemcpyAsync(srec[f].ptr(), hl[f].data(), sizeof(uint32_t) * hl[f].size(), hipMemcpyHostToDevice, st));
    }
    jd.n_pairs = P;
    if (int rc = pn_singles_device(ctx, st, w[0].n_rec, w[1].n_rec, dec, jd, srec[0].as<uint32_t>() + guard, srec[1].as<uint32_t>() + guard, stat.as<uint32_t>() + PS_BLOCK + VS_BLK_WORDS))
        return rc;
    for (int f = 0; f < 2; f++) VS_HIP(ctx, hipMemcpyAsync(hl[f].data(), srec[f].ptr(), sizeof(uint32_t) * hl[f].size(), hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    for (int f = 0; f < 2; f++) {
        for (uint32_t g = 0; g < guard; g++)
            if (hl[f][g] != SENTINEL || hl[f][guard + ns[f] + g] != SENTINEL) return vs_fail(ctx, VS_E_STATE, "%s: a kernel wrote outside the singles list of file %d", who, f + 1);
        if (hl[f][2u * (size_t)guard + ns[f]] != SENTINEL) return vs_fail(ctx, VS_E_STATE, "%s: a kernel wrote outside the singles list of file %d", who, f + 1);
        for (size_t k = 0; k < ns[f]; k++)
            if (hl[f][guard + k] == SENTINEL) return vs_fail(ctx, VS_E_STATE, "%s: a word of the singles list of file %d was not written", who, f + 1);
        const uint64_t take = std::min<uint64_t>(sing->cap[f], ns[f]);
        if (take) memcpy(sing->list[f], hl[f].data() + guard, sizeof(uint32_t) * take);
        info[8 + f] = ns[f];
    }
    return VS_OK;
}

int vs_fastq_join_text(vs_ctx *ctx, const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                       uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, uint32_t guard, uint64_t info[8]) {
    return pn_join_text_entry("vs_fastq_join_text", ctx, text0, n0, text1, n1, eof0, eof1, mode, table, name_bits, pairs, cap_pairs, nullptr, guard, info);
}

int vs_fastq_join_singles_text(vs_ctx *ctx, const uint8_t *text0, uint64_t n0, const uint8_t *text1, uint64_t n1, int eof0, int eof1, int mode, uint32_t table,
                               uint32_t name_bits, uint32_t *pairs, uint64_t cap_pairs, uint32_t *singles0, uint64_t cap_singles0, uint32_t *singles1,
                               uint64_t cap_singles1, uint32_t guard, uint64_t info[10]) {
    const PnSinglesOut sing = {{singles0, singles1}, {cap_singles0, cap_singles1}};
    return pn_join_text_entry("vs_fastq_join_singles_text", ctx, text0, n0, text1, n1, eof0, eof1, mode, table, name_bits, pairs, cap_pairs, &sing, guard, info);
}

}  // extern "C"
