// Interleaved FASTQ ingest: ONE file or pipe in which each pair's two records follow each other (`samtools fastq` to stdout,
// `seqtk mergepe`, `fastp --stdout`; what `bwa mem -p` reads), streamed as vs_stream.hip streams two files -- one Reader, one
// DevWindow, so every form the Reader knows (plain, FIFO, gzip through zlib, BGZF and plain gzip inflated on the device)
// comes with it -- and modelled on the BAM stream (vs_bam.hip): a window is scanned and matched ONCE, blocks are handed out
// from a cursor, the window is cut when its pairs are out.
//
// Which records are mates is decided by NAME, on the device (vs_mates_core.h has the rule): one lost or extra record would
// otherwise shift every later pair by one unnoticed, and `samtools fastq x.bam > out.fq` puts single reads between the pairs.
// Per window (the leftover of the one before + the slot appended):
//   k_sl_count / k_sl_scan / k_sl_scatter   the line ends, as for the two-file stream (vs_stream_lines.h); a flagged window
//                                           ('\r', a byte >= 0x80) goes through host text mode first, names are compared after;
//   k_il_match      one thread per record i: m[i] = mates(i, i + 1), from the two header lines at any byte alignment; the
//                   workgroup's composed parity function (const-0 / const-1 / identity / flip);
//   k_il_carry      one workgroup: the functions of the workgroups composed in order, the parity each workgroup starts with;
//   k_il_classify   one thread per record: its parity from the __ballot of m (consecutive ones below the lane) and the carry,
//                   its class (first / second / single / held back); pair starts per workgroup, singles, the first single;
//   k_sl_scan       pair starts before each workgroup, their total;
//   k_il_emit       rec[2p] = i, rec[2p + 1] = i + 1 for the p-th pair start i.
// A run of ten million equal names is one scan like any other window: nothing walks along it.
// The last complete record of a window that is not the second of a pair waits for its successor (or the end of the file): it
// is held back, unclassified, and leads the next window.  The cut falls behind a consumed record, so the next window starts
// the greedy rule afresh; no parity crosses a cut.
// A block of n pairs from the cursor is cut by the block builder (vs_block_records, vs_reads.hip) from the ends rec[2 cursor ...]
// -- the layout vs_pe_count takes.
// Mode VS_IL_KEEP keeps the single records instead of dropping them: after the window's pairs are listed, k_il_singles_count /
// k_sl_scan / k_il_singles_emit compact the records of class single, in file order, into srec[]; when the pairs of the window
// are out they are handed out as SINGLES blocks (vs_block_singles, the same builder), before the window is cut.  The held-back
// record stays held; at the end of the file it is a single like any other.
// The host reads back counts, the cut and status words; no record text, except the two header lines of the message with
// which the strict mode refuses a single record.
//
// A MEMBER RANGE (vs_fastq_il_open_range; one process per GPU on one whole-BGZF file): the same stream on the members that
// hold a rank's records [a, b) and one look-ahead record, as the two-file stream has it (vs_stream.hip).  Whether record a
// is the second of a pair follows from the parity functions of the shares in front (vs_il_shard_plan chains them); a share's
// function is composed on the device by vs_fastq_il_range_fn: the range streamed through the same reader and window,
// k_il_match per window, then
//   k_il_total      one workgroup: the m of the window's records composed from their ballots, in order, into a running word
//                   on the device -- the TOTAL where k_il_carry gives the prefixes, over exactly the records asked for.
// The window's last record is always carried to lead the next, so every m is computed once from text that is present.
// With entry 1 the range's first record goes unseen, and the record behind it starts with parity 0 like a file's first: no
// parity is handed to a kernel.  The stream sees n_owned + lookahead records and no more; the look-ahead record is held
// back like a window's last record, so it is packed only as the second of the rank's last pair.
#include <algorithm>
#include <string>
#include <vector>

#include "vs_internal.h"
#include "vs_stream_lines.h"
#include "vs_mates_core.h"

#define IL_TPB SL_TPB
#define IL_CARRY_TPB 1024

namespace {

// status words of a stream (the first ST_PER_FILE are the line scanner's)
enum {
    IS_PAIRS = 4, IS_SINGLES = 5, IS_FIRST_SINGLE = 6 /* IL_NONE: none (atomicMin) */, IS_HELD = 7,
    IS_BLOCK = 8,    // the VS_BLK_ST words of the block builder
    IS_WINDOW = 12,  // (words below it are rewritten for every window or block)
    IS_BAD = 12,     // the first BGZF member the device rejected (a running index), ~0u: none
    IS_ALL = 16
};

}  // namespace

// ---- kernels -----------------------------------------------------------------------------------------------------------
// the composed function of the workgroup's wavefronts, in order (thread 0, after the wavefronts wrote theirs)
__device__ __forceinline__ uint32_t il_compose_waves(const uint32_t *wfn, uint32_t upto) {
    uint32_t f = IL_F_ID;
    for (uint32_t w = 0; w < upto; w++) f = il_compose(f, wfn[w]);
    return f;
}

__global__ void __launch_bounds__(IL_TPB) k_il_match(IlWin w, uint8_t *__restrict__ m, uint32_t *__restrict__ wgfn) {
    __shared__ uint32_t wfn[IL_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * IL_TPB + threadIdx.x;
    const bool mi = i + 1u < w.n_rec && il_mates_at(w, i);
    if (i < w.n_rec) m[i] = mi ? 1u : 0u;
    const uint64_t b = __ballot(mi);
    if ((threadIdx.x & (VS_WAVE - 1u)) == 0u) wfn[threadIdx.x / VS_WAVE] = il_wave_fn(b);
    __syncthreads();
    if (threadIdx.x == 0) wgfn[blockIdx.x] = il_compose_waves(wfn, IL_TPB / VS_WAVE);
}

// f[0, n): the function of every workgroup; in place, the parity with which each workgroup starts (the window starts at 0)
__global__ void __launch_bounds__(IL_CARRY_TPB) k_il_carry(uint32_t *__restrict__ f, uint32_t n) {
    __shared__ uint32_t part[IL_CARRY_TPB];
    const uint32_t t = threadIdx.x, per = (n + IL_CARRY_TPB - 1u) / IL_CARRY_TPB;
    const uint32_t lo = min(n, t * per), hi = min(n, lo + per);
    uint32_t own = IL_F_ID;
    for (uint32_t i = lo; i < hi; i++) own = il_compose(own, f[i]);
    part[t] = own;
    __syncthreads();
    for (uint32_t o = 1; o < IL_CARRY_TPB; o <<= 1) {  // inclusive Hillis-Steele; composition is associative, not commutative
        const uint32_t before = t >= o ? part[t - o] : (uint32_t)IL_F_ID;
        __syncthreads();
        part[t] = il_compose(before, part[t]);
        __syncthreads();
    }
    uint32_t p = t ? il_apply(part[t - 1u], 0u) : 0u;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t g = f[i];
        f[i] = p;
        p = il_apply(g, p);
    }
}

// m[0, n): the match flags of n records in a row.  *acc = their composed function after *acc -- the TOTAL where k_il_carry
// gives the prefixes, and over exactly n flags: the lanes that k_il_match pads its last wavefront with are no records here.
// One workgroup; every wavefront composes a contiguous run of 64-record groups from their ballots, thread 0 the wavefronts.
__global__ void __launch_bounds__(IL_CARRY_TPB) k_il_total(const uint8_t *__restrict__ m, uint32_t n, uint32_t *__restrict__ acc) {
    __shared__ uint32_t wfn[IL_CARRY_TPB / VS_WAVE];
    const uint32_t lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    const uint32_t groups = (n + VS_WAVE - 1u) / VS_WAVE, per = (groups + IL_CARRY_TPB / VS_WAVE - 1u) / (IL_CARRY_TPB / VS_WAVE);
    const uint32_t g0 = min(groups, wave * per), g1 = min(groups, g0 + per);
    uint32_t f = IL_F_ID;
    for (uint32_t g = g0; g < g1; g++) {  // (g0, g1 are the wavefront's: every lane takes part in the ballot)
        const uint32_t i = g * VS_WAVE + lane;
        const uint64_t b = __ballot(i < n && m[i] != 0u);
        f = il_compose(f, il_run_fn(b, min((uint32_t)VS_WAVE, n - g * VS_WAVE)));
    }
    if (lane == 0) wfn[wave] = f;
    __syncthreads();
    if (threadIdx.x == 0) *acc = il_compose(*acc, il_compose_waves(wfn, IL_CARRY_TPB / VS_WAVE));
}

__global__ void __launch_bounds__(IL_TPB) k_il_classify(const uint8_t *__restrict__ m, const uint32_t *__restrict__ wg_parity, uint32_t n_rec,
                                                        uint32_t eof, uint8_t *__restrict__ cls, uint32_t *__restrict__ wg_first,
                                                        uint32_t *__restrict__ st) {
    __shared__ uint32_t wfn[IL_TPB / VS_WAVE], wcnt[IL_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * IL_TPB + threadIdx.x, lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    const bool mi = i < n_rec && m[i] != 0u;
    const uint64_t b = __ballot(mi);
    if (lane == 0) wfn[wave] = il_wave_fn(b);
    __syncthreads();
    const uint32_t p_in = il_apply(il_compose_waves(wfn, wave), wg_parity[blockIdx.x]);
    uint32_t c = il_class(il_wave_parity(b, lane, p_in), mi);
    if (i + 1u == n_rec && !eof && c == (uint32_t)IL_SINGLE) {  // (its successor has not been seen)
        c = IL_HELD;
        st[IS_HELD] = 1u;
    }
    if (i < n_rec) cls[i] = (uint8_t)c;
    const uint64_t firsts = __ballot(i < n_rec && c == (uint32_t)IL_FIRST), singles = __ballot(i < n_rec && c == (uint32_t)IL_SINGLE);
    if (lane == 0) {
        wcnt[wave] = (uint32_t)__popcll(firsts);
        if (singles) {
            atomicAdd(&st[IS_SINGLES], (uint32_t)__popcll(singles));
            atomicMin(&st[IS_FIRST_SINGLE], i + (uint32_t)__ffsll((long long)singles) - 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < IL_TPB / VS_WAVE; w++) t += wcnt[w];
        wg_first[blockIdx.x] = t;
    }
}

// wg_base: pair starts in front of every workgroup; rec holds two words for every pair start of the window
__global__ void __launch_bounds__(IL_TPB) k_il_emit(const uint8_t *__restrict__ cls, const uint32_t *__restrict__ wg_base, uint32_t n_rec,
                                                    uint32_t n_pairs, uint32_t *__restrict__ rec) {
    __shared__ uint32_t wcnt[IL_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * IL_TPB + threadIdx.x, lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    const bool first = i < n_rec && cls[i] == (uint8_t)IL_FIRST;
    const uint64_t b = __ballot(first);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!first) return;
    uint32_t p = wg_base[blockIdx.x] + (uint32_t)__popcll(b & (lane ? (~0ull >> (VS_WAVE - lane)) : 0ull));
    for (uint32_t w = 0; w < wave; w++) p += wcnt[w];
    if (p >= n_pairs) return;  // (cannot be: the total of the scan is n_pairs)
    rec[2u * p] = i;
    rec[2u * p + 1u] = i + 1u;
}

// VS_IL_KEEP: the single records of each workgroup counted (wg_cnt, scanned afterwards), then srec[q] = i for the q-th single
// record i of the window -- a ballot and the counts of the wavefronts in front, as k_il_emit places the pair starts
__global__ void __launch_bounds__(IL_TPB) k_il_singles_count(const uint8_t *__restrict__ cls, uint32_t n_rec, uint32_t *__restrict__ wg_cnt) {
    __shared__ uint32_t wcnt[IL_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * IL_TPB + threadIdx.x;
    const uint64_t b = __ballot(i < n_rec && cls[i] == (uint8_t)IL_SINGLE);
    if ((threadIdx.x & (VS_WAVE - 1u)) == 0u) wcnt[threadIdx.x / VS_WAVE] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < IL_TPB / VS_WAVE; w++) t += wcnt[w];
        wg_cnt[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(IL_TPB) k_il_singles_emit(const uint8_t *__restrict__ cls, const uint32_t *__restrict__ wg_base, uint32_t n_rec,
                                                            uint32_t n_singles, uint32_t *__restrict__ srec) {
    __shared__ uint32_t wcnt[IL_TPB / VS_WAVE];
    const uint32_t i = blockIdx.x * IL_TPB + threadIdx.x, lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    const bool single = i < n_rec && cls[i] == (uint8_t)IL_SINGLE;
    const uint64_t b = __ballot(single);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!single) return;
    uint32_t q = wg_base[blockIdx.x] + (uint32_t)__popcll(b & (lane ? (~0ull >> (VS_WAVE - lane)) : 0ull));
    for (uint32_t w = 0; w < wave; w++) q += wcnt[w];
    if (q >= n_singles) return;  // (cannot be: the total of the scan is n_singles)
    srec[q] = i;
}

// ---- the match of one window ------------------------------------------------------------------------------------------------
namespace {

struct IlMatch {
    VsDevBuf m, cls;          // uint8 per record: the match flag with the record behind it, the class
    VsDevBuf wgfn, wg_first;  // uint32 per workgroup: parity function -> parity at its start; pair starts -> those in front
    VsDevBuf rec;             // uint32: rec[2p], rec[2p + 1] = the records of the window's p-th pair
    VsDevBuf srec, wg_single; // VS_IL_KEEP: srec[q] = the window's q-th single record; singles per workgroup -> those in front
    uint32_t n_rec = 0, n_pairs = 0, singles = 0, first_single = IL_NONE, decided = 0;
    bool held = false;
};

// Records [0, n_rec) of the window (txt, its line ends scattered) classified: counts into mt (synchronises the stream).
// d_stat / h_stat: IS_ALL status words, [IS_PAIRS, IS_BLOCK) rewritten.
int il_classify_device(vs_ctx *ctx, hipStream_t st, const uint8_t *txt, const uint32_t *ends, uint32_t n_rec, bool eof, IlMatch &mt, uint32_t *d_stat,
                       uint32_t *h_stat) {
    const uint32_t wgs = (n_rec + IL_TPB - 1u) / IL_TPB;
    mt.n_rec = n_rec;
    mt.n_pairs = mt.singles = mt.decided = 0;
    mt.first_single = IL_NONE;
    mt.held = false;
    if (!n_rec) return VS_OK;
    if (int rc = reserve_n<uint8_t>(ctx, mt.m, n_rec)) return rc;
    if (int rc = reserve_n<uint8_t>(ctx, mt.cls, n_rec)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, mt.wgfn, wgs)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, mt.wg_first, (size_t)wgs + 1u)) return rc;
    VS_HIP(ctx, hipMemsetAsync(d_stat + IS_PAIRS, 0, sizeof(uint32_t) * (IS_BLOCK - IS_PAIRS), st));
    VS_HIP(ctx, hipMemsetAsync(d_stat + IS_FIRST_SINGLE, 0xFF, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_il_match, dim3(wgs), dim3(IL_TPB), 0, st, IlWin{txt, ends, n_rec}, mt.m.as<uint8_t>(), mt.wgfn.as<uint32_t>());
    hipLaunchKernelGGL(k_il_carry, dim3(1), dim3(IL_CARRY_TPB), 0, st, mt.wgfn.as<uint32_t>(), wgs);
    hipLaunchKernelGGL(k_il_classify, dim3(wgs), dim3(IL_TPB), 0, st, mt.m.as<const uint8_t>(), mt.wgfn.as<const uint32_t>(), n_rec, eof ? 1u : 0u,
                       mt.cls.as<uint8_t>(), mt.wg_first.as<uint32_t>(), d_stat);
    VS_HIP(ctx, hipGetLastError());
    vs_launch_scan_u32(st, mt.wg_first.as<uint32_t>(), wgs, d_stat + IS_PAIRS);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(h_stat + IS_PAIRS, d_stat + IS_PAIRS, sizeof(uint32_t) * (IS_BLOCK - IS_PAIRS), hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    mt.n_pairs = h_stat[IS_PAIRS];
    mt.singles = h_stat[IS_SINGLES];
    mt.first_single = h_stat[IS_FIRST_SINGLE];
    mt.held = h_stat[IS_HELD] != 0u;
    mt.decided = n_rec - (mt.held ? 1u : 0u);
    if (2ull * mt.n_pairs + mt.singles != mt.decided) return vs_fail(ctx, VS_E_STATE, "the classes of an interleaved window do not add up to its records");
    return VS_OK;
}

// the pair list of a classified window into rec (2 mt.n_pairs words)
int il_emit_device(vs_ctx *ctx, hipStream_t st, const IlMatch &mt, uint32_t *rec) {
    if (!mt.n_pairs) return VS_OK;
    hipLaunchKernelGGL(k_il_emit, dim3((mt.n_rec + IL_TPB - 1u) / IL_TPB), dim3(IL_TPB), 0, st, mt.cls.as<const uint8_t>(), mt.wg_first.as<const uint32_t>(),
                       mt.n_rec, mt.n_pairs, rec);
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

// VS_IL_KEEP: the single records of a classified window listed in srec (mt.singles words), in file order.  d_total: a status
// word for the scan's total (synchronises nothing)
int il_emit_singles_device(vs_ctx *ctx, hipStream_t st, IlMatch &mt, uint32_t *d_total) {
    if (!mt.singles) return VS_OK;
    const uint32_t wgs = (mt.n_rec + IL_TPB - 1u) / IL_TPB;
    if (int rc = reserve_n<uint32_t>(ctx, mt.wg_single, (size_t)wgs + 1u)) return rc;
    if (int rc = reserve_n<uint32_t>(ctx, mt.srec, (size_t)mt.singles)) return rc;
    hipLaunchKernelGGL(k_il_singles_count, dim3(wgs), dim3(IL_TPB), 0, st, mt.cls.as<const uint8_t>(), mt.n_rec, mt.wg_single.as<uint32_t>());
    vs_launch_scan_u32(st, mt.wg_single.as<uint32_t>(), wgs, d_total);
    hipLaunchKernelGGL(k_il_singles_emit, dim3(wgs), dim3(IL_TPB), 0, st, mt.cls.as<const uint8_t>(), mt.wg_single.as<const uint32_t>(), mt.n_rec, mt.singles,
                       mt.srec.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    return VS_OK;
}

void il_mates_info(uint64_t info[6], uint64_t pairs, uint64_t singles, uint64_t decided, bool held, uint32_t first_single, uint64_t records) {
    info[0] = pairs;
    info[1] = singles;
    info[2] = decided;
    info[3] = held ? decided : ~0ull;
    info[4] = first_single == IL_NONE ? ~0ull : first_single;
    info[5] = records;
}

}  // namespace

// ---- the stream ------------------------------------------------------------------------------------------------------------
struct vs_fastq_il : StreamState {  // (IS_ALL status words)
    int device = 0;
    hipStream_t st = nullptr;
    Reader rd;
    DevFile df;  // the one window, its line ends
    IlMatch mt;
    bool matched = false;   // mt describes the window
    uint32_t pair_cur = 0;  // the first pair of the matched window not yet delivered
    uint32_t single_cur = 0;  // VS_IL_KEEP: the first single record of the matched window not yet delivered
    bool singles_ok = false;
    bool keep = false;  // VS_IL_KEEP: the single records are handed out as singles blocks
    VsDevBuf d_wcnt;
    uint64_t pairs = 0, singles = 0, records = 0;
    uint32_t flags_seen = 0;
    // a member range (vs_fastq_il_open_range): records of the range not yet decided; the last of them is the next rank's
    // first (look-ahead); the range's first record is the second of the previous rank's last pair and goes unseen; the
    // window that holds the range's last record has been matched
    bool ranged = false, lookahead = false, entry_pending = false, range_done = false;
    uint64_t remain = 0;
};

namespace {

// count + scan of the window: its line ends counted, flags, records (synchronises the stream)
int il_scan(vs_ctx *ctx, vs_fastq_il *s) {
    DevFile &d = s->df;
    VS_HIP(ctx, hipMemsetAsync(s->d_stat, 0, sizeof(uint32_t) * ST_PER_FILE, s->st));
    if (int rc = reserve_n<uint32_t>(ctx, d.wg, sl_workgroups(d.w.size) + 1u)) return rc;
    vs_launch_sl_count(s->st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), s->d_stat);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(s->h_stat, s->d_stat, sizeof(uint32_t) * IS_ALL, hipMemcpyDeviceToHost, s->st));
    VS_HIP(ctx, hipStreamSynchronize(s->st));
    d.take_status(s->h_stat);
    s->flags_seen |= d.flags;
    return VS_OK;
}

// the header line of record r of the window, for a message (at most 200 bytes of it)
std::string il_header_line(vs_fastq_il *s, uint32_t r) {
    uint32_t e[2] = {0, 0};
    const uint32_t *ends = s->df.ends.as<const uint32_t>();
    if (r && hipMemcpy(&e[0], ends + 4u * (size_t)r - 1u, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return "?";
    if (hipMemcpy(&e[1], ends + 4u * (size_t)r, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return "?";
    const size_t a = r ? (size_t)e[0] + 1u : 0u, b = e[1];
    if (a > b || b > s->df.w.size) return "?";
    std::string line(std::min<size_t>(b - a, 200u), '\0');
    if (!line.empty() && hipMemcpy(&line[0], s->df.w.data() + a, line.size(), hipMemcpyDeviceToHost) != hipSuccess) return "?";
    return line;
}

// the end of the input: the reader's failure, if it had one
int il_finish(vs_ctx *ctx, vs_fastq_il *s) {
    if (s->rd.err != VS_OK) return s->fail(ctx, s->rd.err, s->rd.err_msg);
    s->done = true;
    return VS_OK;
}

// the first n_lines lines of the scanned window (`records` complete records) dropped: its line ends scattered once, the
// offset of the last one to drop read back (synchronises the stream)
int il_drop_lines(vs_ctx *ctx, vs_fastq_il *s, uint64_t n_lines, uint64_t records) {
    DevFile &d = s->df;
    if (d.n_nl < n_lines) return vs_fail(ctx, VS_E_STATE, "%s: fewer lines at the front of its member range than were counted", s->rd.path.c_str());
    if (int rc = reserve_n<uint32_t>(ctx, d.ends, (size_t)d.n_nl + 1u)) return rc;
    vs_launch_sl_scatter(s->st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), d.ends.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    uint32_t at = 0;
    VS_HIP(ctx, hipMemcpyAsync(&at, d.ends.as<uint32_t>() + (n_lines - 1u), sizeof at, hipMemcpyDeviceToHost, s->st));
    VS_HIP(ctx, hipStreamSynchronize(s->st));
    if ((size_t)at + 1u > d.w.size) return vs_fail(ctx, VS_E_STATE, "%s: a line end beyond the window", s->rd.path.c_str());
    return drop_front(ctx, s->st, d, (size_t)at + 1u, records);
}

// One more slot appended to the window and the window scanned.  A member range starts inside a record of the rank before:
// the lines in front that belong to it go (they all end in the range's first member -- that is how the plan picks it -- and
// a slot holds whole members, so the first window has them).
int il_append(vs_ctx *ctx, vs_fastq_il *s) {
    DevFile &d = s->df;
    {
        SlotLease taken;  // (goes back once the stream is synchronised: the upload is done)
        if (int rc = append_chunk(ctx, s->st, d, s->rd, taken, s->d_stat + IS_BAD)) return rc;
        if (int rc = il_scan(ctx, s)) return rc;
        if (taken) (void)member_failed(d, s->rd, *taken, s->h_stat[IS_BAD]);
    }
    if (!s->ranged || d.err != VS_OK) return VS_OK;
    // (pass 1 of the sharded open saw neither a '\r' nor a byte >= 0x80 in the whole file, and the plan rests on that)
    if (d.flags) return vs_fail(ctx, VS_E_STATE, "%s changed after its lines were counted", s->rd.path.c_str());
    if (!d.skip) return VS_OK;
    if (int rc = il_drop_lines(ctx, s, d.skip, 0)) return rc;
    d.skip = 0;
    return il_scan(ctx, s);
}

// The next window: the decided records of the last one cut off, a slot appended, the line ends found, the records matched.
// *end: nothing more comes (the stream is done or has failed; the code is returned).
int il_next_window(vs_ctx *ctx, vs_fastq_il *s, bool *end) {
    DevFile &d = s->df;
    hipStream_t st = s->st;
    *end = true;
    if (s->matched) {
        if (d.eof || s->range_done) return il_finish(ctx, s);
        size_t cut = 0;
        if (s->mt.decided) {  // one past the line end that closes the last decided record
            uint32_t at = 0;
            VS_HIP(ctx, hipMemcpyAsync(&at, d.ends.as<uint32_t>() + (4u * (size_t)s->mt.decided - 1u), sizeof at, hipMemcpyDeviceToHost, st));
            VS_HIP(ctx, hipStreamSynchronize(st));
            cut = (size_t)at + 1u;
            if (cut > d.w.size) return s->fail(ctx, VS_E_STATE, s->rd.path + ": a line end beyond the window");
        }
        if (int rc = drop_front(ctx, st, d, cut, s->mt.decided)) return s->fail(ctx, rc, vs_last_error(ctx));
        s->matched = false;
        s->pair_cur = 0;
        s->single_cur = 0;
    }
    for (;;) {
        if (int rc = il_append(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
        if (d.err == VS_OK && d.flags && d.validated < d.w.size) {  // (text that arrived with this slot: host text mode)
            if (translate_window(ctx, d, s->rd.path) == VS_OK)
                if (int rc = il_scan(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
        }
        if (d.err != VS_OK) return s->fail(ctx, s->rd.err != VS_OK ? s->rd.err : d.err, s->rd.err != VS_OK ? s->rd.err_msg : d.err_msg);
        if (!s->entry_pending) break;
        // the range's first record is the SECOND of the previous rank's last pair: it goes as soon as it is whole, uncounted,
        // and the record behind the second of a pair starts with parity 0 like a file's first
        if (d.records) {
            int rc = il_drop_lines(ctx, s, 4u, 1u);
            if (rc == VS_OK) rc = il_scan(ctx, s);
            if (rc) return s->fail(ctx, rc, vs_last_error(ctx));
            s->entry_pending = false;
            s->remain--;
            break;
        }
        if (d.eof) return s->fail(ctx, VS_E_STATE, s->rd.path + ": fewer records in its member range than were counted");
    }
    uint32_t n_rec = (uint32_t)d.records;
    bool eof = d.eof;
    if (s->ranged) {  // (the stream sees the range's records and no more: behind the last one the file may go on)
        if (d.records >= s->remain) {
            n_rec = (uint32_t)s->remain;
            eof = !s->lookahead;  // (a look-ahead record is held back unless it completes this rank's last pair)
            s->range_done = true;
        } else if (d.eof) {
            return s->fail(ctx, VS_E_STATE, s->rd.path + ": fewer records in its member range than were counted");
        }
    }
    if (int rc = reserve_n<uint32_t>(ctx, d.ends, (size_t)d.n_nl + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
    vs_launch_sl_scatter(st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), d.ends.as<uint32_t>());
    if (int rc = il_classify_device(ctx, st, d.w.data(), d.ends.as<const uint32_t>(), n_rec, eof, s->mt, s->d_stat, s->h_stat))
        return s->fail(ctx, rc, vs_last_error(ctx));
    s->matched = true;
    if (!s->singles_ok && s->mt.first_single != IL_NONE) {
        const uint32_t r = s->mt.first_single;
        const std::string next = r + 1u < s->mt.n_rec ? "\"" + il_header_line(s, r + 1u) + "\"" : std::string("end of file");
        return s->fail(ctx, VS_E_ARG,
                       s->rd.path + ": record " + std::to_string(d.first_record + r) + " (\"" + il_header_line(s, r) + "\") has no mate beside it: what follows it is " +
                           next + ".  An interleaved FASTQ holds the two records of a pair one behind the other under one name; to drop and count "
                                  "single records, add --interleaved-singles");
    }
    if (int rc = reserve_n<uint32_t>(ctx, s->mt.rec, 2u * (size_t)s->mt.n_pairs + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
    if (int rc = il_emit_device(ctx, st, s->mt, s->mt.rec.as<uint32_t>())) return s->fail(ctx, rc, vs_last_error(ctx));
    if (s->keep)
        if (int rc = il_emit_singles_device(ctx, st, s->mt, s->d_stat + IS_BLOCK + VS_BLK_WORDS)) return s->fail(ctx, rc, vs_last_error(ctx));
    s->records += s->mt.decided;
    s->singles += s->mt.singles;
    if (s->ranged) s->remain -= s->mt.decided;
    *end = false;
    return VS_OK;
}

// the file opened and its reader started; range (may be NULL) = {first byte, one past the last byte, lines to skip}.  start =
// false: no reader is started (a range without a record of this rank's)
int il_open(vs_ctx *ctx, const char *path, int mode, const uint64_t *range, bool start, vs_fastq_il **out) {
    *out = nullptr;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    vs_fastq_il *s = new vs_fastq_il();
    s->device = ctx->device;
    s->singles_ok = mode != VS_IL_STRICT;
    s->keep = mode == VS_IL_KEEP;
    Reader &r = s->rd;
    fastq_switches(r, range != nullptr, s->df.w.gz.text_cap);
    int rc = r.open_file(ctx, path);
    struct stat sb;
    if (rc == VS_OK && range && (fstat(r.fd, &sb) != 0 || !S_ISREG(sb.st_mode) || range[0] > range[1] || range[1] > (uint64_t)sb.st_size))
        rc = r.cannot_open(ctx, EINVAL);  // (a member range is a range of a regular file that holds it)
    if (rc != VS_OK) {
        delete s;
        return rc;
    }
    if (range) {
        s->ranged = true;
        // (a short range -- the few members of a tail pass -- pins no slots of the full chunk size: deflate rarely packs text
        // eightfold, and a slot holds at least one member whatever its size)
        r.chunk = (size_t)std::min<uint64_t>(r.chunk, std::max<uint64_t>(1u << 20, 8u * (range[1] - range[0])));
        r.begin = range[0];
        r.end = range[1];
        s->df.skip = range[2];
        s->df.to_file_end = r.end == (uint64_t)sb.st_size;
    }
    hipError_t e1 = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e1 == hipSuccess) e1 = s->reserve_stat(IS_ALL);
    if (e1 == hipSuccess) e1 = hipMemset(s->d_stat + IS_BAD, 0xFF, sizeof(uint32_t));
    if (e1 != hipSuccess) {
        vs_fastq_il_close(s);
        return vs_fail(ctx, VS_E_HIP, "vs_fastq_il_open: %s", hipGetErrorString(e1));
    }
    if (start) r.th = std::thread([rp = &s->rd] { rp->run(); });
    else s->done = true;
    *out = s;
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_fastq_il_open(vs_ctx *ctx, const char *path, int mode, vs_fastq_il **out) {
    if (!ctx || !path || !out || (mode != VS_IL_STRICT && mode != VS_IL_SINGLES && mode != VS_IL_KEEP)) return vs_fail(ctx, VS_E_ARG, "vs_fastq_il_open: bad argument");
    return il_open(ctx, path, mode, nullptr, true, out);
}

int vs_fastq_il_open_range(vs_ctx *ctx, const char *path, int mode, const uint64_t range[3], uint64_t n_owned, int lookahead, uint32_t entry,
                           uint64_t first_record, vs_fastq_il **out) {
    if (!ctx || !path || !range || !out || (mode != VS_IL_STRICT && mode != VS_IL_SINGLES) || (lookahead != 0 && lookahead != 1) || entry > 1u ||
        n_owned > (1ull << 60))
        return vs_fail(ctx, VS_E_ARG, "vs_fastq_il_open_range: bad argument");
    const bool any = n_owned > entry;  // (a share that is empty, or only the second of the previous rank's last pair: nothing is read)
    if (int rc = il_open(ctx, path, mode, range, any, out)) return rc;
    vs_fastq_il *s = *out;
    s->lookahead = lookahead != 0;
    s->entry_pending = any && entry != 0u;
    s->remain = any ? n_owned + (uint64_t)lookahead : 0u;
    s->df.first_record = first_record;
    return VS_OK;
}

int vs_fastq_il_range_fn(vs_ctx *ctx, const char *path, const uint64_t range[3], uint64_t n_rec, uint32_t *fn, uint64_t info[4]) {
    if (!ctx || !path || !range || !fn || !info || n_rec > (1ull << 60)) return vs_fail(ctx, VS_E_ARG, "vs_fastq_il_range_fn: bad argument");
    *fn = IL_F_ID;
    info[0] = info[1] = info[2] = info[3] = 0;
    if (n_rec < 2u) return VS_OK;  // (no two records in a row: nothing to compose, nothing is read)
    vs_fastq_il *s = nullptr;
    if (int rc = il_open(ctx, path, VS_IL_SINGLES, range, true, &s)) return rc;
    // the function so far between two sentinel words: d_acc[1], composed on the device window by window
    const uint32_t SENTINEL = 0xA5C3F00Du, start[3] = {SENTINEL, IL_F_ID, SENTINEL};
    uint32_t got[3] = {0, 0, 0};
    VsDevBuf acc, m, wgfn;
    DevFile &d = s->df;
    hipStream_t st = s->st;
    uint64_t seen = 0, windows = 0;  // records in front of the window; windows matched
    auto done = [&](int rc) {
        s->rd.shut();  // (the reader has stopped: its byte count stands)
        info[0] = d.w.members;
        info[1] = s->rd.raw_bytes;
        info[2] = windows;
        info[3] = seen;
        vs_fastq_il_close(s);
        return rc;
    };
    hipError_t e1 = acc.reserve(sizeof start);
    if (e1 == hipSuccess) e1 = hipMemcpyAsync(acc.ptr(), start, sizeof start, hipMemcpyHostToDevice, st);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
    if (e1 != hipSuccess) return done(vs_fail(ctx, VS_E_HIP, "vs_fastq_il_range_fn: %s", hipGetErrorString(e1)));
    for (;;) {
        if (int rc = il_append(ctx, s)) return done(rc);
        if (d.err != VS_OK) return done(vs_fail(ctx, s->rd.err != VS_OK ? s->rd.err : d.err, "%s", (s->rd.err != VS_OK ? s->rd.err_msg : d.err_msg).c_str()));
        // records [seen, seen + n) of the range are whole in the window; the last of them only lends its header line to the
        // m of the one before and leads the next window
        const uint64_t n = std::min<uint64_t>(d.records, n_rec - seen);
        if (n < 2u) {
            if (d.eof) return done(vs_fail(ctx, VS_E_STATE, "%s: fewer records in its member range than were counted", path));
            continue;  // (the window grows)
        }
        const uint32_t wgs = (uint32_t)((n + IL_TPB - 1u) / IL_TPB);
        if (int rc = reserve_n<uint32_t>(ctx, d.ends, (size_t)d.n_nl + 1u)) return done(rc);
        if (int rc = reserve_n<uint8_t>(ctx, m, (size_t)n)) return done(rc);
        if (int rc = reserve_n<uint32_t>(ctx, wgfn, wgs)) return done(rc);
        vs_launch_sl_scatter(st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), d.ends.as<uint32_t>());
        hipLaunchKernelGGL(k_il_match, dim3(wgs), dim3(IL_TPB), 0, st, IlWin{d.w.data(), d.ends.as<const uint32_t>(), (uint32_t)n}, m.as<uint8_t>(),
                           wgfn.as<uint32_t>());
        hipLaunchKernelGGL(k_il_total, dim3(1), dim3(IL_CARRY_TPB), 0, st, m.as<const uint8_t>(), (uint32_t)(n - 1u), acc.as<uint32_t>() + 1);
        if ((e1 = hipGetLastError()) != hipSuccess) return done(vs_fail(ctx, VS_E_HIP, "vs_fastq_il_range_fn: %s", hipGetErrorString(e1)));
        windows++;
        seen += n - 1u;
        if (seen + 1u == n_rec) break;
        uint32_t at = 0;  // one past the line end that closes record n - 2 of the window (the stream's own wait per window)
        e1 = hipMemcpyAsync(&at, d.ends.as<uint32_t>() + (4u * (size_t)(n - 1u) - 1u), sizeof at, hipMemcpyDeviceToHost, st);
        if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
        if (e1 != hipSuccess) return done(vs_fail(ctx, VS_E_HIP, "vs_fastq_il_range_fn: %s", hipGetErrorString(e1)));
        if ((size_t)at + 1u > d.w.size) return done(vs_fail(ctx, VS_E_STATE, "%s: a line end beyond the window", path));
        if (int rc = drop_front(ctx, st, d, (size_t)at + 1u, n - 1u)) return done(rc);
    }
    seen++;  // (the last record, whose header line was read)
    e1 = hipMemcpyAsync(got, acc.ptr(), sizeof got, hipMemcpyDeviceToHost, st);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);
    if (e1 != hipSuccess) return done(vs_fail(ctx, VS_E_HIP, "vs_fastq_il_range_fn: %s", hipGetErrorString(e1)));
    if (got[0] != SENTINEL || got[2] != SENTINEL || got[1] > 3u) return done(vs_fail(ctx, VS_E_STATE, "vs_fastq_il_range_fn: a kernel wrote outside the function word"));
    *fn = got[1];
    return done(VS_OK);
}

int vs_il_shard_plan(const uint32_t *fn, uint32_t world, uint32_t *entry) {
    if (!fn || !entry || !world) return vs_fail(nullptr, VS_E_ARG, "vs_il_shard_plan: bad argument");
    uint32_t e = 0;  // (the file's first record starts with parity 0)
    for (uint32_t r = 0; r < world; r++) {
        if (fn[r] > 3u) return vs_fail(nullptr, VS_E_ARG, "vs_il_shard_plan: the function of rank %u is none of the four", r);
        entry[r] = e;
        e = il_apply(fn[r], e);
    }
    return VS_OK;
}

int vs_fastq_il_next(vs_ctx *ctx, vs_fastq_il *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs) {
    if (!ctx || !s || !out || !n_pairs) return vs_fail(ctx, VS_E_ARG, "vs_fastq_il_next: bad argument");
    *out = nullptr;
    *n_pairs = 0;
    if (s->failed != VS_OK) return s->again(ctx);
    if (s->done) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    if (!max_pairs || max_pairs > (1ull << 30)) max_pairs = 1ull << 30;
    while (!s->matched || (s->pair_cur >= s->mt.n_pairs && !(s->keep && s->single_cur < s->mt.singles))) {
        bool end = false;
        const int rc = il_next_window(ctx, s, &end);
        if (end) return rc;
    }
    DevFile &d = s->df;
    // ---- the block of n pairs from the cursor -- or, VS_IL_KEEP and the window's pairs out, a singles block of n of its single
    // records: rec[i] = the record of the block's i-th end / read
    const bool single = s->pair_cur >= s->mt.n_pairs;
    const uint64_t n = std::min<uint64_t>(single ? s->mt.singles - s->single_cur : s->mt.n_pairs - s->pair_cur, max_pairs);
    const uint32_t *rec = single ? s->mt.srec.as<const uint32_t>() + s->single_cur : s->mt.rec.as<const uint32_t>() + 2u * (size_t)s->pair_cur;
    const SlWin win = {d.w.data(), d.ends.as<const uint32_t>(), d.n_nl, (uint32_t)d.w.size};
    const VsBlockJob job = {ctx, s->st, 2u * n, &s->d_wcnt, s->d_stat + IS_BLOCK, s->h_stat + IS_BLOCK, VS_BLK_ST, false};
    vs_reads *r = nullptr;
    const hipError_t e1 = single ? vs_block_singles(job, win, rec, 0u, &r) : vs_block_records(job, win, rec, &r);
    if (e1 != hipSuccess) return s->fail_hip(ctx, "vs_fastq_il_next", e1);
    if (!r) {  // (neither source faults an end: the end is over the limit)
        const uint32_t e = s->h_stat[IS_BLOCK + VS_BLK_BAD] & ~VS_BLK_OVER;
        return s->fail(ctx, VS_E_RANGE, too_long_line(s->rd.path, d.first_record + fetch_u32(rec + (single ? e >> 1 : e))));
    }
    if (single) s->single_cur += (uint32_t)n;
    else s->pair_cur += (uint32_t)n, s->pairs += n;
    *out = r;
    *n_pairs = n;
    return VS_OK;
}

int vs_fastq_il_info(const vs_fastq_il *s, uint64_t info[6]) {
    if (!s || !info) return VS_E_ARG;
    info[0] = s->pairs;
    info[1] = s->singles;
    info[2] = s->records;
    info[3] = s->rd.text_bytes + s->df.w.gz.text;
    info[4] = s->rd.raw_bytes;
    info[5] = (uint64_t)s->flags_seen | (s->rd.gzip ? 4u : 0u) | (s->done ? 16u : 0u);
    return VS_OK;
}

void vs_fastq_il_close(vs_fastq_il *s) {
    if (!s) return;
    s->rd.shut();
    if (s->st) (void)hipStreamSynchronize(s->st);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

// ---- test aids: the match of one window -----------------------------------------------------------------------------------
int vs_fastq_mates_host(const uint8_t *text, uint64_t n, int eof, uint32_t *pairs, uint64_t cap_pairs, uint64_t info[6]) {
    if ((!text && n) || !info || (!pairs && cap_pairs) || n > STREAM_MAX_WINDOW) return vs_fail(nullptr, VS_E_ARG, "vs_fastq_mates_host: bad argument");
    std::vector<uint32_t> ends;
    for (uint64_t i = 0; i < n; i++)
        if (text[i] == '\n') ends.push_back((uint32_t)i);
    const uint64_t lines = ends.size() + ((eof && n && text[n - 1u] != '\n') ? 1u : 0u);
    const uint32_t n_rec = (uint32_t)(lines / 4u);
    ends.push_back((uint32_t)n);  // (never read: a complete record's header and sequence lines have line ends of their own)
    const IlWin w = {text, ends.data(), n_rec};
    uint64_t n_pairs = 0, singles = 0;
    uint32_t parity = 0, first_single = IL_NONE;
    bool held = false;
    for (uint32_t i = 0; i < n_rec; i++) {
        const bool m = i + 1u < n_rec && il_mates_at(w, i);
        const uint32_t c = il_class(parity, m);
        parity = il_step(parity, m);
        if (c == (uint32_t)IL_FIRST) {
            if (n_pairs < cap_pairs) pairs[2u * n_pairs] = i, pairs[2u * n_pairs + 1u] = i + 1u;
            n_pairs++;
        } else if (c == (uint32_t)IL_SINGLE) {
            if (i + 1u == n_rec && !eof) {
                held = true;
                continue;
            }
            if (first_single == IL_NONE) first_single = i;
            singles++;
        }
    }
    il_mates_info(info, n_pairs, singles, n_rec - (held ? 1u : 0u), held, first_single, n_rec);
    return VS_OK;
}

int vs_fastq_mates_text(vs_ctx *ctx, const uint8_t *text, uint64_t n, int eof, uint32_t *pairs, uint64_t cap_pairs, uint32_t guard, uint64_t info[6]) {
    if (!ctx || (!text && n) || !info || (!pairs && cap_pairs) || n > STREAM_MAX_WINDOW || guard > (1u << 20))
        return vs_fail(ctx, VS_E_ARG, "vs_fastq_mates_text: bad argument");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t wgs = sl_workgroups(n);
    const uint32_t SENTINEL = 0xA5C3F00Du;
    VsDevBuf txt, wg, ends, stat, rec;
    IlMatch mt;
    uint32_t hs[IS_ALL] = {0};
    VS_HIP(ctx, txt.reserve(DevWindow::padded(n)));
    VS_HIP(ctx, wg.reserve(sizeof(uint32_t) * (wgs + 1u)));
    VS_HIP(ctx, stat.reserve(sizeof(uint32_t) * IS_ALL));
    VS_HIP(ctx, hipMemsetAsync(stat.ptr(), 0, sizeof(uint32_t) * IS_ALL, st));
    if (n) VS_HIP(ctx, hipMemcpyAsync(txt.ptr(), text, n, hipMemcpyHostToDevice, st));
    vs_launch_sl_count(st, txt.as<const uint8_t>(), n, wg.as<uint32_t>(), stat.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(hs, stat.ptr(), sizeof(uint32_t) * ST_PER_FILE, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t lines = (uint64_t)hs[ST_NL] + ((eof && n && hs[ST_LAST] != '\n') ? 1u : 0u);
    const uint32_t n_rec = (uint32_t)(lines / 4u);
    VS_HIP(ctx, ends.reserve(sizeof(uint32_t) * ((size_t)hs[ST_NL] + 1u)));
    vs_launch_sl_scatter(st, txt.as<const uint8_t>(), n, wg.as<const uint32_t>(), ends.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    if (int rc = il_classify_device(ctx, st, txt.as<const uint8_t>(), ends.as<const uint32_t>(), n_rec, eof != 0, mt, stat.as<uint32_t>(), hs)) return rc;
    // the pair list between two rows of `guard` sentinel words
    const size_t body = 2u * (size_t)mt.n_pairs, all = body + 2u * (size_t)guard;
    std::vector<uint32_t> h(all ? all : 1u, SENTINEL);
    VS_HIP(ctx, rec.reserve(sizeof(uint32_t) * (all ? all : 1u)));
    if (all) VS_HIP(ctx, hipMemcpyAsync(rec.ptr(), h.data(), sizeof(uint32_t) * all, hipMemcpyHostToDevice, st));
    if (int rc = il_emit_device(ctx, st, mt, rec.as<uint32_t>() + guard)) return rc;
    if (all) VS_HIP(ctx, hipMemcpyAsync(h.data(), rec.ptr(), sizeof(uint32_t) * all, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    for (uint32_t g = 0; g < guard; g++)
        if (h[g] != SENTINEL || h[guard + body + g] != SENTINEL) return vs_fail(ctx, VS_E_STATE, "vs_fastq_mates_text: a kernel wrote outside the pair list");
    for (size_t k = 0; k < body; k++)
        if (h[guard + k] == SENTINEL) return vs_fail(ctx, VS_E_STATE, "vs_fastq_mates_text: a word of the pair list was not written");
    const uint64_t np = std::min<uint64_t>(cap_pairs, mt.n_pairs);
    if (np) memcpy(pairs, h.data() + guard, sizeof(uint32_t) * 2u * np);
    il_mates_info(info, mt.n_pairs, mt.singles, mt.decided, mt.held, mt.first_single, n_rec);
    return VS_OK;
}

}  // extern "C"
