// Streamed FASTQ ingest: both files read front to back through a bounded ring of pinned chunks, the records found and
// packed ON THE DEVICE.  For inputs the mapped ingest (vs_fastq.hip) cannot take: a FIFO, /dev/stdin or a process
// substitution has no size to map, and a gzip file is inflated there whole into memory before anything is counted.
//
// Host: one reader thread per file (the Reader of vs_stream_reader.h, which the BAM ingest shares) read(2)s any fd -- inflating with zlib in streaming mode when the file starts with
// the gzip magic (several members in a row are fine; a cut-off stream or trailing bytes that are no member are VS_E_ARG,
// as in map_file) -- into a ring of STREAM_RING_SLOTS pinned chunks of STREAM_CHUNK_BYTES.  Peak host memory is the
// ring, whatever the size of the file.
//
// BGZF (the blocked gzip of bgzip / htslib / samtools; VS_BGZF_DEVICE=0 switches this off): when a file's first bytes
// are a BGZF member the reader does not inflate.  It fills a slot with the raw deflate payloads of WHOLE members, their
// directory (payload offset and length, output offset, ISIZE, CRC32) growing down from the slot's end, until the ISIZE sum
// would pass the chunk size or the slot is full; the device inflates them into the window (k_inflate of vs_inflate.hip,
// one wavefront per member) and checks every CRC32.  The index of the first member that failed comes back with the
// statistics scan_windows reads anyway.  A slot holds at least one member whatever VS_STREAM_CHUNK says, so the ring's
// pinned memory is STREAM_RING_SLOTS x max(chunk, 64 KiB) per file.  From the first byte that is no whole BGZF member
// (another gzip member, garbage, a member cut off by the end of the file) the file goes through the zlib loop for the rest
// of it -- which also words the failure for what is no gzip at all.  A member the device rejected is inflated again with
// zlib on the host for the code of that message; should zlib accept it, that is VS_E_STATE, never a silent continuation.
//
// PLAIN GZIP ON THE DEVICE (VS_GZIP_DEVICE=1, off by default): a file that starts with the gzip magic and whose first member
// is not BGZF is one deflate stream, or a few, without a directory.  The reader then makes no zlib call: its slots carry the
// file's bytes as they are (Slot::gz), and DevWindow::append_gzip decodes them behind the window in parallel -- block starts
// found speculatively, runs counted, chained and decoded into symbols, histories handed down, symbols resolved, every
// member's CRC32 and ISIZE checked (vs_gzip.hip, vs_gzip_core.h); what cannot finish inside a slot is carried to the next.
// A slot may add no text at all (it ended inside the first run): the round loop then simply takes the next one.  A stream
// the device refuses fails the file in the words of the zlib loop: gzip_failed reads a regular file again with zlib for the
// code; a pipe's message names the device's status instead.
//
// Device: every file has a window = the bytes left over from the last block (they start at a record boundary) + the
// chunks appended since.  Per step, for each window:
//   k_sl_count    one lane per 16-byte word: newlines per workgroup, flags for '\r' and bytes >= 0x80, the last byte;
//   k_sl_scan     exclusive scan of the workgroup counts (one workgroup);
//   k_sl_scatter  the lane's rank among the newlines of its wavefront from __ballot, + its wavefront's and workgroup's
//                 base: the byte offset of every line end;
// then, for the n = min(complete records of fwd, of rve) pairs of the block:
//   k_sl_cut      the record cuts behind the block, one thread per file;
// and from there on as every block of a streamed ingest is built, by the block builder (build_block of vs_reads.hip, here
// vs_block_lines): k_block_ends, length (line 4r+1 minus its newline) and packed words of every end; k_sl_scan, word offsets;
// k_pack_reads, one thread per packed word, straight from the windows, the mask beside the words; k_count_invalid, and k_inv4
// when some end needs it.  The block is the layout vs_pe_count takes.
//
// A window whose scan raises a flag ('\r' or a byte >= 0x80) keeps the reference's text-mode semantics on the host
// (rare): its complete lines are copied back, universal newlines applied ("\r\n" and a lone '\r' end a line; a '\r' at
// the end of the window waits for the next chunk, which may start with '\n'), every multi-byte UTF-8 character becomes
// one '?' (seq_chars), the bytes are checked with utf8_range_ok, and the text goes back to the device to be scanned
// again.  Plain ASCII with LF line ends never passes through host parsing.
//
// A MEMBER RANGE (vs_fastq_stream_open_range; one process per GPU on two whole-BGZF files): the same stream on the bytes
// [first member, one past the last member) of each file.  The reader seeks to the first and never reads at or beyond the
// second; the device drops the lines in front that belong to the neighbour's record (skip_lines) and the stream ends
// after the rank's pairs.  Which range that is follows from per-member line counts that the ranks made on their devices
// and exchanged before (vs_bgzf_walk_file, vs_bgzf_count_lines, further down; the plan is vs_bgzf_shard_plan of
// vs_inflate.hip).  A final line without a newline counts only where the range ends with the file.
//
// What ONE file needs of all this -- its window and line ends (DevFile), a slot appended in each form, host text mode, the
// wording of a rejected stream or member -- is in vs_stream_lines.h, which the interleaved ingest (vs_interleaved.hip) shares.
#include <errno.h>
#include <fcntl.h>
#include <poll.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "vs_internal.h"
#include "vs_stream_lines.h"

#define SL_SCAN_TPB 1024

namespace {

// per-window status the kernels write (one uint32 array per stream, read back in one copy)
// ([f * ST_PER_FILE + ST_NL / ST_FLAGS / ST_LAST]: vs_stream_lines.h)
enum { ST_BLOCK = 8 /* the VS_BLK_ST words of the block builder */, ST_CUT = 12 /* + f: behind them, read back with them */, ST_N = 16 };
enum { ST_BAD = ST_N /* + f: the first member of file f the device rejected (a running index), ~0u: none */, ST_ALL = ST_N + 2 };

}  // namespace

// ---- kernels -----------------------------------------------------------------------------------------------------------
// exact mask (0x80 per byte) of the bytes of x equal to c
__device__ __forceinline__ uint32_t sl_eq(uint32_t x, uint32_t c4) {
    const uint32_t t = x ^ c4;
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}

// the 16 bytes of word wi (bytes at or beyond n read as 0)
__device__ __forceinline__ uint4 sl_load16(const uint8_t *txt, uint64_t n, uint64_t wi) {
    const uint64_t b = wi * 16u;
    uint4 v = *(const uint4 *)(txt + b);  // (the window buffer is padded to whole words)
    if (b + 16u > n) {
        const uint32_t keep = (uint32_t)(n - b);  // 0..15
        uint32_t *p = (uint32_t *)&v;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t lo = 4u * k;
            p[k] = keep >= lo + 4u ? p[k] : keep <= lo ? 0u : p[k] & ((1u << (8u * (keep - lo))) - 1u);
        }
    }
    return v;
}

__device__ __forceinline__ uint32_t sl_nl_mask(const uint4 v, uint32_t out[4]) {
    const uint32_t *p = (const uint32_t *)&v;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        out[k] = sl_eq(p[k], 0x0A0A0A0Au);
        c += (uint32_t)__popc(out[k]);
    }
    return c;
}

// newlines per workgroup, flags of the window, its last byte
__global__ void __launch_bounds__(SL_TPB) k_sl_count(const uint8_t *__restrict__ txt, uint64_t n, uint32_t *__restrict__ wg_cnt,
                                                     uint32_t *__restrict__ st) {
    __shared__ uint32_t wsum[SL_TPB / VS_WAVE];
    const uint64_t wi = (uint64_t)blockIdx.x * SL_TPB + threadIdx.x;
    uint32_t c = 0, fl = 0;
    if (wi * 16u < n) {
        const uint4 v = sl_load16(txt, n, wi);
        uint32_t m[4];
        c = sl_nl_mask(v, m);
        const uint32_t *p = (const uint32_t *)&v;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (sl_eq(p[k], 0x0D0D0D0Du)) fl |= FL_CR;
            if (p[k] & 0x80808080u) fl |= FL_HIGH;
        }
        if (wi * 16u + 16u >= n) st[ST_LAST] = txt[n - 1u];  // (the lane that holds the window's last byte)
    }
    const uint32_t lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    uint32_t s = c;
#pragma unroll
    for (uint32_t o = VS_WAVE / 2u; o; o >>= 1) s += __shfl_xor(s, o);
    const bool any_cr = __ballot(fl & FL_CR) != 0ull, any_high = __ballot(fl & FL_HIGH) != 0ull;
    if (lane == 0) {
        wsum[wave] = s;
        if (any_cr || any_high) atomicOr(&st[ST_FLAGS], (any_cr ? FL_CR : 0u) | (any_high ? FL_HIGH : 0u));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < SL_TPB / VS_WAVE; w++) t += wsum[w];
        wg_cnt[blockIdx.x] = t;
    }
}

// exclusive scan of a[0, m) in place, one workgroup; the total to *total (uint32: the callers' totals are below 2^32)
__global__ void __launch_bounds__(SL_SCAN_TPB) k_sl_scan(uint32_t *__restrict__ a, uint32_t m, uint32_t *__restrict__ total) {
    __shared__ uint32_t part[SL_SCAN_TPB];
    const uint32_t t = threadIdx.x, per = (m + SL_SCAN_TPB - 1u) / SL_SCAN_TPB;
    const uint32_t lo = min(m, t * per), hi = min(m, lo + per);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += a[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t o = 1; o < SL_SCAN_TPB; o <<= 1) {  // inclusive Hillis-Steele over the thread sums
        const uint32_t add = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t x = a[i];
        a[i] = run;
        run += x;
    }
    if (t == SL_SCAN_TPB - 1u) *total = part[t];
}
void vs_launch_scan_u32(hipStream_t st, uint32_t *a, uint32_t m, uint32_t *total) {
    hipLaunchKernelGGL(k_sl_scan, dim3(1), dim3(SL_SCAN_TPB), 0, st, a, m, total);
}

// the byte offset of every newline, in order: workgroup base (scanned counts) + wavefront base + the lane's rank, the
// rank from __ballot of the bits of every lane's count
__global__ void __launch_bounds__(SL_TPB) k_sl_scatter(const uint8_t *__restrict__ txt, uint64_t n, const uint32_t *__restrict__ wg_base,
                                                       uint32_t *__restrict__ ends) {
    __shared__ uint32_t wsum[SL_TPB / VS_WAVE];
    const uint64_t wi = (uint64_t)blockIdx.x * SL_TPB + threadIdx.x;
    uint32_t c = 0, m[4] = {0u, 0u, 0u, 0u};
    if (wi * 16u < n) c = sl_nl_mask(sl_load16(txt, n, wi), m);
    const uint32_t lane = threadIdx.x & (VS_WAVE - 1u), wave = threadIdx.x / VS_WAVE;
    const uint64_t below = lane ? (~0ull >> (VS_WAVE - lane)) : 0ull;
    uint32_t rank = 0, wtotal = 0;
#pragma unroll
    for (uint32_t b = 0; b < 5; b++) {  // c <= 16: five bits
        const uint64_t bal = __ballot((c >> b) & 1u);
        rank += (uint32_t)__popcll(bal & below) << b;
        wtotal += (uint32_t)__popcll(bal) << b;
    }
    if (lane == 0) wsum[wave] = wtotal;
    __syncthreads();
    uint32_t base = wg_base[blockIdx.x];
    for (uint32_t w = 0; w < wave; w++) base += wsum[w];
    if (!c) return;
    uint32_t at = base + rank;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        uint32_t mk = m[k];
        while (mk) {
            const uint32_t bit = (uint32_t)__ffs((int)mk) - 1u;  // 7, 15, 23 or 31
            ends[at++] = (uint32_t)(wi * 16u) + 4u * k + (bit >> 3);
            mk &= mk - 1u;
        }
    }
}

void vs_launch_sl_count(hipStream_t st, const uint8_t *txt, uint64_t n, uint32_t *wg, uint32_t *stat) {
    const uint64_t wgs = sl_workgroups(n);
    if (!wgs) return;
    hipLaunchKernelGGL(k_sl_count, dim3((unsigned)wgs), dim3(SL_TPB), 0, st, txt, n, wg, stat);
    hipLaunchKernelGGL(k_sl_scan, dim3(1), dim3(SL_SCAN_TPB), 0, st, wg, (uint32_t)wgs, stat + ST_NL);
}
void vs_launch_sl_scatter(hipStream_t st, const uint8_t *txt, uint64_t n, const uint32_t *wg, uint32_t *ends) {
    const uint64_t wgs = sl_workgroups(n);
    if (wgs) hipLaunchKernelGGL(k_sl_scatter, dim3((unsigned)wgs), dim3(SL_TPB), 0, st, txt, n, wg, ends);
}

// two threads, one per file: the record cut behind a block of n_pairs pairs (one past the newline of line 4 n_pairs - 1)
__global__ void __launch_bounds__(VS_WAVE) k_sl_cut(SlWin f0, SlWin f1, uint32_t n_pairs, uint32_t *__restrict__ cut) {
    if (threadIdx.x >= 2u) return;
    const SlWin &w = threadIdx.x ? f1 : f0;
    const uint32_t last = 4u * n_pairs - 1u;
    cut[threadIdx.x] = last < w.n_nl ? w.ends[last] + 1u : w.size;
}

// ---- host side (the reader: vs_stream_reader.h; one file's window and line ends: DevFile of vs_stream_lines.h) -------------
struct vs_fastq_stream : StreamState {  // (ST_ALL status words)
    int device = 0;
    hipStream_t st = nullptr;
    Reader rd[2];
    DevFile df[2];
    VsDevBuf d_wcnt;  // uint32
    uint64_t pairs = 0;
    uint64_t limit = ~0ull;  // pairs to deliver (a member range: the rank's own)
    bool ranged = false;
    uint32_t flags_seen = 0;
};

namespace {

// count + scan of window f: n_nl, flags, last byte into the host status (synchronises the stream)
int scan_windows(vs_ctx *ctx, vs_fastq_stream *s, int only = -1) {
    hipStream_t st = s->st;
    VS_HIP(ctx, hipMemsetAsync(s->d_stat, 0, sizeof(uint32_t) * ST_N, st));
    for (int f = 0; f < 2; f++) {
        if (only >= 0 && f != only) continue;
        DevFile &d = s->df[f];
        if (int rc = reserve_n<uint32_t>(ctx, d.wg, sl_workgroups(d.w.size) + 1u)) return rc;
        vs_launch_sl_count(st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), s->d_stat + f * ST_PER_FILE);
    }
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(s->h_stat, s->d_stat, sizeof(uint32_t) * ST_ALL, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    for (int f = 0; f < 2; f++) {
        if (only >= 0 && f != only) continue;
        DevFile &d = s->df[f];
        d.take_status(s->h_stat + f * ST_PER_FILE);
        s->flags_seen |= d.flags;
    }
    return VS_OK;
}

// the end-of-input check of bytes that were never parsed (the rest of the longer file): valid UTF-8, a character cut by
// a chunk boundary carried to the next piece
bool check_piece(DevFile &d, const uint8_t *p, size_t n, bool last) {
    std::vector<uint8_t> tmp;
    if (d.n_pend) {
        for (uint32_t i = 0; i < d.n_pend; i++) tmp.push_back((uint8_t)d.pend[i]);
        tmp.insert(tmp.end(), p, p + n);
        p = tmp.data();
        n = tmp.size();
        d.n_pend = 0;
    }
    size_t upto = n;
    if (!last) {  // a lead byte in the last three whose character does not fit: wait for the next piece
        for (size_t j = n; j-- > 0 && n - j <= 3u;) {
            const uint8_t c = p[j];
            if ((c & 0xC0u) == 0x80u) continue;
            if (c >= 0xC0u) {
                const size_t len = c >= 0xF0u ? 4u : c >= 0xE0u ? 3u : 2u;
                if (j + len > n) upto = j;
            }
            break;
        }
    }
    bool high = false;
    for (size_t i = 0; i < upto && !high; i++) high = p[i] >= 0x80u;
    if (high && !vs_utf8_range_ok(p, upto, 0, upto)) return false;
    for (size_t i = upto; i < n; i++) d.pend[d.n_pend++] = p[i];
    return true;
}

// Both files to their ends (the reference reads them whole): every byte not yet checked is checked, a reader's failure is
// picked up; then the first failure in file order.
int finish(vs_ctx *ctx, vs_fastq_stream *s) {
    for (int f = 0; f < 2; f++) {
        DevFile &d = s->df[f];
        Reader &r = s->rd[f];
        if (d.err == VS_OK && d.validated < d.w.size && (d.flags & FL_HIGH)) {
            std::vector<uint8_t> buf(d.w.size - d.validated);
            VS_HIP(ctx, hipMemcpy(buf.data(), d.w.data() + d.validated, buf.size(), hipMemcpyDeviceToHost));
            if (!check_piece(d, buf.data(), buf.size(), d.eof)) {
                d.err = VS_E_UTF8;
                d.err_msg = r.path + " holds bytes that are not valid UTF-8 (the reference's text-mode read raises UnicodeDecodeError)";
            }
        }
        d.validated = d.w.size;
        while (!d.eof) {
            if (d.err == VS_OK && d.w.gz.more) {  // held-back gzip runs: a round on them, no slot
                d.w.size = 0;
                int rc = append_gzip(ctx, s->st, d, r, nullptr);
                if (rc == VS_OK) rc = scan_windows(ctx, s, f);
                if (rc != VS_OK) return s->fail(ctx, rc, vs_last_error(ctx));
                if (d.err == VS_OK && ((d.flags & FL_HIGH) || d.n_pend)) {
                    std::vector<uint8_t> buf(d.w.size);
                    if (d.w.size && hipMemcpy(buf.data(), d.w.data(), d.w.size, hipMemcpyDeviceToHost) != hipSuccess)
                        return s->fail(ctx, VS_E_HIP, "vs_fastq_stream_next: copying a window back failed");
                    if (!check_piece(d, buf.data(), buf.size(), d.eof)) {
                        d.err = VS_E_UTF8;
                        d.err_msg = r.path + " holds bytes that are not valid UTF-8 (the reference's text-mode read raises UnicodeDecodeError)";
                    }
                }
                d.w.size = d.validated = 0;
                continue;
            }
            const SlotLease lease(r);  // (goes back at the end of the round, or with a failure)
            const Slot &sl = *lease;
            bool ok = true;
            if (d.err == VS_OK && (sl.comp || sl.gz)) {
                // no text on the host: the members are inflated (and their CRCs checked) on the device like any others, and
                // the text comes back only when the scan saw a byte >= 0x80 (or a character is still open)
                d.w.size = 0;
                int rc = append_slot(ctx, s->st, d, r, sl, s->d_stat + ST_BAD + f);
                if (rc == VS_OK) rc = scan_windows(ctx, s, f);
                if (rc != VS_OK) {
                    return s->fail(ctx, rc, vs_last_error(ctx));
                }
                if (!member_failed(d, r, sl, s->h_stat[ST_BAD + f]) && d.err == VS_OK && ((d.flags & FL_HIGH) || d.n_pend)) {
                    std::vector<uint8_t> buf(d.w.size);
                    if (d.w.size && hipMemcpy(buf.data(), d.w.data(), d.w.size, hipMemcpyDeviceToHost) != hipSuccess)
                        return s->fail(ctx, VS_E_HIP, "vs_fastq_stream_next: copying a window back failed");
                    ok = check_piece(d, buf.data(), buf.size(), sl.gz ? d.eof : sl.last);
                }
                d.w.size = d.validated = 0;
            } else if (d.err == VS_OK) {
                ok = check_piece(d, sl.buf.as<uint8_t>(), sl.len, sl.last);
            }
            if (!ok) {
                d.err = VS_E_UTF8;
                d.err_msg = r.path + " holds bytes that are not valid UTF-8 (the reference's text-mode read raises UnicodeDecodeError)";
            }
            d.eof = sl.last && !(d.err == VS_OK && d.w.gz.more);
        }
        if (d.err == VS_OK && d.n_pend) {  // (a character cut off by the end of the file)
            d.err = VS_E_UTF8;
            d.err_msg = r.path + " holds bytes that are not valid UTF-8 (the reference's text-mode read raises UnicodeDecodeError)";
        }
        if (r.err != VS_OK) {  // (a read or gzip failure comes before what the bytes say: map_file fails first)
            d.err = r.err;
            d.err_msg = r.err_msg;
        }
    }
    s->done = true;
    for (int f = 0; f < 2; f++)
        if (s->df[f].err != VS_OK) return s->fail(ctx, s->df[f].err, s->df[f].err_msg);
    return VS_OK;
}

// A member range starts inside a record of the rank before: after scan_windows, the first d.skip lines of the window of
// file f go (its line ends scattered once, the offset of the last one to drop read back).  They all end in the range's
// first member -- that is how the plan picks it -- and a slot holds whole members, so the first window has them.
int skip_lines(vs_ctx *ctx, vs_fastq_stream *s, int f) {
    DevFile &d = s->df[f];
    if (d.n_nl < d.skip) return vs_fail(ctx, VS_E_STATE, "%s: fewer lines at the front of its member range than were counted", s->rd[f].path.c_str());
    if (int rc = reserve_n<uint32_t>(ctx, d.ends, (size_t)d.n_nl + 1u)) return rc;
    vs_launch_sl_scatter(s->st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), d.ends.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    uint32_t at = 0;
    VS_HIP(ctx, hipMemcpyAsync(&at, d.ends.as<uint32_t>() + (d.skip - 1u), sizeof at, hipMemcpyDeviceToHost, s->st));
    VS_HIP(ctx, hipStreamSynchronize(s->st));
    if ((size_t)at + 1u > d.w.size) return vs_fail(ctx, VS_E_STATE, "%s: a line end beyond the window", s->rd[f].path.c_str());
    d.skip = 0;
    return drop_front(ctx, s->st, d, (size_t)at + 1u, 0);
}

// both files opened and their readers started; range (may be NULL) = per file {first byte, one past the last byte, lines to skip}
int stream_open(vs_ctx *ctx, const char *fwd_path, const char *rve_path, const uint64_t *range, uint64_t n_pairs, vs_fastq_stream **out) {
    *out = nullptr;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    vs_fastq_stream *s = new vs_fastq_stream();
    s->device = ctx->device;
    const char *paths[2] = {fwd_path, rve_path};
    for (int f = 0; f < 2; f++) {
        Reader &r = s->rd[f];
        fastq_switches(r, range != nullptr, s->df[f].w.gz.text_cap);
        int rc = r.open_file(ctx, paths[f]);
        struct stat sb;
        if (rc == VS_OK && range && (fstat(r.fd, &sb) != 0 || !S_ISREG(sb.st_mode) || range[3 * f] > range[3 * f + 1] || range[3 * f + 1] > (uint64_t)sb.st_size))
            rc = r.cannot_open(ctx, EINVAL);  // (a member range is a range of a regular file that holds it)
        if (rc != VS_OK) {
            for (int g = 0; g < f; g++) close(s->rd[g].fd);
            for (int g = 0; g < 2; g++) s->rd[g].fd = -1;
            delete s;
            return rc;
        }
        if (range) {
            r.begin = range[3 * f];
            r.end = range[3 * f + 1];
            s->df[f].skip = range[3 * f + 2];
            s->df[f].to_file_end = r.end == (uint64_t)sb.st_size;
        }
    }
    if (range) {
        s->ranged = true;
        s->limit = n_pairs;
    }
    hipError_t e1 = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e1 == hipSuccess) e1 = s->reserve_stat(ST_ALL);
    if (e1 == hipSuccess) e1 = hipMemset(s->d_stat + ST_BAD, 0xFF, sizeof(uint32_t) * 2);
    if (e1 != hipSuccess) {
        vs_fastq_stream_close(s);
        return vs_fail(ctx, VS_E_HIP, "vs_fastq_stream_open: %s", hipGetErrorString(e1));
    }
    for (int f = 0; f < 2; f++) s->rd[f].th = std::thread([r = &s->rd[f]] { r->run(); });
    *out = s;
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_fastq_stream_open(vs_ctx *ctx, const char *fwd_path, const char *rve_path, vs_fastq_stream **out) {
    if (!ctx || !fwd_path || !rve_path || !out) return vs_fail(ctx, VS_E_ARG, "vs_fastq_stream_open: bad argument");
    return stream_open(ctx, fwd_path, rve_path, nullptr, 0, out);
}

int vs_fastq_stream_open_range(vs_ctx *ctx, const char *fwd_path, const char *rve_path, const uint64_t range[6], uint64_t n_pairs,
                               vs_fastq_stream **out) {
    if (!ctx || !fwd_path || !rve_path || !range || !out) return vs_fail(ctx, VS_E_ARG, "vs_fastq_stream_open_range: bad argument");
    return stream_open(ctx, fwd_path, rve_path, range, n_pairs, out);
}

int vs_fastq_stream_next(vs_ctx *ctx, vs_fastq_stream *s, uint64_t max_pairs, vs_reads **out, uint64_t *n_pairs) {
    if (!ctx || !s || !out || !n_pairs) return vs_fail(ctx, VS_E_ARG, "vs_fastq_stream_next: bad argument");
    *out = nullptr;
    *n_pairs = 0;
    if (s->failed != VS_OK) return s->again(ctx);
    if (s->done) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    if (!max_pairs || max_pairs > (1ull << 30)) max_pairs = 1ull << 30;
    if (s->pairs >= s->limit) return finish(ctx, s);  // (a member range: the rank's pairs are out)
    max_pairs = std::min<uint64_t>(max_pairs, s->limit - s->pairs);
    uint64_t n = 0;
    for (int round = 0;; round++) {
        // more text for the file that holds fewer complete records (both at the start): a window holds what is left of the
        // last block + one chunk, so its size stays bounded whatever the two files' record lengths
        SlotLease taken[2];  // (a failure gives them back)
        bool fresh[2] = {false, false};
        for (int f = 0; f < 2; f++) {
            DevFile &d = s->df[f], &o = s->df[f ^ 1];
            const bool need = !d.eof && d.records < max_pairs && d.records <= o.records && !(o.eof && o.records <= d.records);
            if (!need) continue;
            if (int rc = append_chunk(ctx, s->st, d, s->rd[f], taken[f], s->d_stat + ST_BAD + f)) return s->fail(ctx, rc, vs_last_error(ctx));
            fresh[f] = true;
        }
        if (round > 0 && !fresh[0] && !fresh[1]) return finish(ctx, s);  // (nothing more to read and no pair: the end)
        int rc = scan_windows(ctx, s);
        if (rc) return s->fail(ctx, rc, vs_last_error(ctx));
        bool rejected = false;
        for (int f = 0; f < 2; f++)
            if (fresh[f] && ((taken[f] && member_failed(s->df[f], s->rd[f], *taken[f], s->h_stat[ST_BAD + f])) || s->df[f].err != VS_OK)) rejected = true;  // (needs the slot: before it goes back)
        for (int f = 0; f < 2; f++) taken[f].give_back();  // (the stream is synchronised: the upload is done)
        if (rejected) return finish(ctx, s);
        if (s->ranged) {
            // (pass 1 of the sharded open saw neither a '\r' nor a byte >= 0x80 in the whole file, and the plan rests on that)
            if (s->df[0].flags | s->df[1].flags)
                return s->fail(ctx, VS_E_STATE, s->rd[s->df[0].flags ? 0 : 1].path + " changed after its lines were counted");
            bool skipped = false;
            for (int f = 0; f < 2; f++) {
                if (!s->df[f].skip || !fresh[f]) continue;  // (the first window of the file; it may arrive a round after the other's)
                if ((rc = skip_lines(ctx, s, f))) return s->fail(ctx, rc, vs_last_error(ctx));
                skipped = true;
            }
            if (skipped && (rc = scan_windows(ctx, s))) return s->fail(ctx, rc, vs_last_error(ctx));
        }
        bool again = false;
        for (int f = 0; f < 2; f++) {
            DevFile &d = s->df[f];
            if (fresh[f] && d.flags && d.validated < d.w.size) {  // (text that arrived with this chunk: host text mode)
                if (translate_window(ctx, d, s->rd[f].path) != VS_OK) return finish(ctx, s);
                again = true;
            }
        }
        if (again && (rc = scan_windows(ctx, s))) return s->fail(ctx, rc, vs_last_error(ctx));
        n = std::min(std::min(s->df[0].records, s->df[1].records), max_pairs);
        if (n > 0) break;
        if ((s->df[0].eof && s->df[0].records == 0) || (s->df[1].eof && s->df[1].records == 0)) return finish(ctx, s);
    }
    // ---- the block of n pairs
    hipStream_t st = s->st;
    const uint64_t n_ends = 2u * n;
    for (int f = 0; f < 2; f++) {
        DevFile &d = s->df[f];
        if (int rc = reserve_n<uint32_t>(ctx, d.ends, (size_t)d.n_nl + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
        vs_launch_sl_scatter(st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), d.ends.as<uint32_t>());
    }
    SlWin w0 = {s->df[0].w.data(), s->df[0].ends.as<uint32_t>(), s->df[0].n_nl, (uint32_t)s->df[0].w.size};
    SlWin w1 = {s->df[1].w.data(), s->df[1].ends.as<uint32_t>(), s->df[1].n_nl, (uint32_t)s->df[1].w.size};
    // the record cuts ride back with the builder's words; the windows are cut behind the block, so the last wait is here
    hipLaunchKernelGGL(k_sl_cut, dim3(1), dim3(VS_WAVE), 0, st, w0, w1, (uint32_t)n, s->d_stat + ST_CUT);
    const VsBlockJob job = {ctx, st, n_ends, &s->d_wcnt, s->d_stat + ST_BLOCK, s->h_stat + ST_BLOCK, VS_BLK_ST + 2u, true};
    vs_reads *r = nullptr;
    hipError_t e1 = vs_block_lines(job, w0, w1, &r);
    if (e1 != hipSuccess) return s->fail_hip(ctx, "vs_fastq_stream_next", e1);
    if (!r) {  // (the source faults no end: the end is over the limit)
        const uint32_t e = s->h_stat[ST_BLOCK + VS_BLK_BAD] & ~VS_BLK_OVER;
        return s->fail(ctx, VS_E_RANGE, too_long_line(s->rd[e & 1u].path, s->df[e & 1u].first_record + (e >> 1)));
    }
    for (int f = 0; f < 2 && e1 == hipSuccess; f++)
        if (drop_front(ctx, st, s->df[f], s->h_stat[ST_CUT + f], n) != VS_OK) e1 = hipErrorOutOfMemory;
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(st);  // (the block is complete when it is handed out)
    if (e1 != hipSuccess) {
        vs_reads_free(ctx, r);
        return s->fail_hip(ctx, "vs_fastq_stream_next", e1);
    }
    s->pairs += n;
    *out = r;
    *n_pairs = n;
    return VS_OK;
}

int vs_fastq_stream_info(const vs_fastq_stream *s, uint64_t info[4]) {
    if (!s || !info) return VS_E_ARG;
    info[0] = s->pairs;
    info[1] = s->rd[0].text_bytes + s->rd[1].text_bytes + s->df[0].w.gz.text + s->df[1].w.gz.text;
    info[2] = s->rd[0].raw_bytes + s->rd[1].raw_bytes;
    info[3] = (uint64_t)s->flags_seen | (s->rd[0].gzip ? 4u : 0u) | (s->rd[1].gzip ? 8u : 0u) | (s->done ? 16u : 0u);
    return VS_OK;
}

void vs_fastq_stream_close(vs_fastq_stream *s) {
    if (!s) return;
    for (Reader &r : s->rd) r.shut();
    if (s->st) (void)hipStreamSynchronize(s->st);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

int vs_fastq_stream_inflate_info(const vs_fastq_stream *s, uint64_t info[4]) {
    if (!s || !info) return VS_E_ARG;
    for (int f = 0; f < 2; f++) {
        info[2 * f + 0] = s->df[f].w.members;
        info[2 * f + 1] = s->rd[f].members_host;
    }
    return VS_OK;
}

int vs_fastq_stream_gzip_info(const vs_fastq_stream *s, uint64_t info[8]) {
    if (!s || !info) return VS_E_ARG;
    for (int f = 0; f < 2; f++) {
        const GzStream &g = s->df[f].w.gz;
        info[4 * f + 0] = g.windows;
        info[4 * f + 1] = g.runs;
        info[4 * f + 2] = g.dropped;
        info[4 * f + 3] = g.members;
    }
    return VS_OK;
}

// ---- the member-sharded open of a BGZF pair (one process per GPU), pass 1 ------------------------------------------------
// The header hop: only the header (and the 8-byte trailer, for ISIZE) of every member is read, never a payload.
int vs_bgzf_walk_file(const char *path, uint64_t *offsets, uint64_t cap, uint64_t info[4]) {
    if (!path || !info || (!offsets && cap)) return vs_fail(nullptr, VS_E_ARG, "vs_bgzf_walk_file: bad argument");
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return vs_fail(nullptr, VS_E_ARG, "cannot open %s: %s", path, strerror(errno));
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        close(fd);
        return vs_fail(nullptr, VS_E_ARG, "%s is not a regular file", path);
    }
    const uint64_t size = (uint64_t)sb.st_size;
    std::vector<uint8_t> head(12u + 65535u);
    uint64_t at = 0, count = 0;
    int state = 0;
    while (at < size) {
        size_t have = 0, hsize = 0, msize = 0;
        for (size_t want = 64;;) {  // (bgzip's header is 18 bytes; a longer extra field is read to its end, 12 + XLEN, and no further)
            want = (size_t)std::min<uint64_t>(want, size - at);
            if (const char *why = pread_all(fd, head.data() + have, want - have, at + have)) {
                close(fd);
                return vs_fail(nullptr, VS_E_ARG, "cannot read %s: %s", path, why);
            }
            have = want;
            state = vs_bgzf_header(head.data(), have, &hsize, &msize);
            const size_t whole = have >= 12 ? 12u + ((size_t)head[10] | ((size_t)head[11] << 8)) : 12u;
            if (state != 1 || whole <= have || at + have == size) break;
            want = whole;
        }
        if (state == 0 && at + msize > size) state = 1;  // cut off by the end of the file
        if (state == 0) {
            uint8_t t[4];
            if (const char *why = pread_all(fd, t, 4, at + msize - 4)) {
                close(fd);
                return vs_fail(nullptr, VS_E_ARG, "cannot read %s: %s", path, why);
            }
            const uint32_t isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
            if (isize > 65536u) state = 2;
        }
        if (state) break;
        if (count < cap) offsets[count] = at;
        count++;
        at += msize;
    }
    close(fd);
    if (count < cap) offsets[count] = at;  // (one past the last member)
    info[0] = count;
    info[1] = at;
    info[2] = (uint64_t)state;
    info[3] = size;
    return VS_OK;
}

int vs_bgzf_count_lines(vs_ctx *ctx, const char *path, const uint64_t *offsets, uint64_t n, uint32_t *counts, uint64_t info[4]) {
    if (!ctx || !path || !info || (n && (!offsets || !counts))) return vs_fail(ctx, VS_E_ARG, "vs_bgzf_count_lines: bad argument");
    info[0] = info[2] = info[3] = 0;
    info[1] = 256;
    if (!n) return VS_OK;
    for (uint64_t i = 0; i < n; i++)
        if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > 65536u) return vs_fail(ctx, VS_E_ARG, "vs_bgzf_count_lines: member %llu is no BGZF member's size", (unsigned long long)i);
    VS_HIP(ctx, hipSetDevice(ctx->device));
    constexpr size_t BATCH = 32u << 20;  // compressed bytes per launch; two pinned buffers of it, one device copy
    struct FdGuard {
        int fd;
        ~FdGuard() { if (fd >= 0) close(fd); }
    } file = {open(path, O_RDONLY)};
    if (file.fd < 0) return vs_fail(ctx, VS_E_ARG, "cannot open %s: %s", path, strerror(errno));
    hipStream_t st = ctx->stream;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n, (uint64_t)std::max(ctx->n_cu, 1) * 8u);
    VsPinnedBuf pin[2];
    VsDevBuf d_comp, d_dir, d_res, d_scratch;
    VS_HIP(ctx, d_comp.reserve(BATCH + 16u));
    VS_HIP(ctx, d_scratch.reserve((size_t)grid * 65536u));
    std::vector<vs_bgzf_member> dir[2];
    VsPinnedBuf pin_dir[2], pin_res[2];  // (pinned, so that neither copy makes the host wait for the kernel before it)
    uint64_t first[2] = {0, 0}, next = 0;
    struct SyncGuard {  // (no return while the device may still read or write this call's buffers)
        hipStream_t st;
        ~SyncGuard() { (void)hipStreamSynchronize(st); }
    } drain = {st};
    for (int k = 0; next < n || !dir[k ^ 1].empty(); k ^= 1) {
        dir[k].clear();
        size_t bytes = 0;
        if (next < n) {  // read and parse batch k while the device still works on the one before
            uint64_t upto = next;
            while (upto < n && offsets[upto + 1] - offsets[next] <= BATCH) upto++;
            bytes = (size_t)(offsets[upto] - offsets[next]);
            VS_HIP(ctx, pin[k].reserve(BATCH));
            uint8_t *buf = pin[k].as<uint8_t>();
            if (const char *why = pread_all(file.fd, buf, bytes, offsets[next])) return vs_fail(ctx, VS_E_ARG, "cannot read %s: %s", path, why);
            for (uint64_t i = next; i < upto; i++) {
                vs_bgzf_member mb;
                size_t msize = 0;
                const size_t rel = (size_t)(offsets[i] - offsets[next]);
                if (vs_bgzf_parse(buf + rel, (size_t)(offsets[i + 1] - offsets[i]), &mb, &msize) != 0 || msize != offsets[i + 1] - offsets[i])
                    return vs_fail(ctx, VS_E_STATE, "%s: no BGZF member of %llu bytes at byte %llu (the file changed after it was walked?)", path,
                                   (unsigned long long)(offsets[i + 1] - offsets[i]), (unsigned long long)offsets[i]);
                mb.in_off += (uint32_t)rel;
                dir[k].push_back(mb);
            }
            first[k] = next;
            next = upto;
            info[3] += bytes;
        }
        const int o = k ^ 1;
        if (!dir[o].empty()) {  // the batch before: its results
            VS_HIP(ctx, hipStreamSynchronize(st));
            for (size_t i = 0; i < dir[o].size(); i++) {
                const uint32_t *r = pin_res[o].as<uint32_t>() + 4u * i;
                if (r[0] != 0) {  // worded as the streamed ingest words a member its device rejected (member_failed)
                    int rc = Z_DATA_ERROR;
                    if (zlib_accepts(pin[o].as<uint8_t>() + dir[o][i].in_off, dir[o][i], &rc))
                        return vs_fail(ctx, VS_E_STATE, "%s: BGZF member %llu was rejected on the device (status %u) but zlib accepts it", path,
                                       (unsigned long long)(first[o] + i), r[0]);
                    return vs_fail(ctx, VS_E_ARG, "%s: not a complete gzip stream (zlib code %d)", path, rc);
                }
                counts[first[o] + i] = r[1];
                info[0] |= r[2];
                if (dir[o][i].isize) info[1] = r[3] & 255u;
            }
            info[2] += dir[o].size();
            dir[o].clear();
        }
        if (!dir[k].empty()) {
            const size_t nm = dir[k].size();
            VS_HIP(ctx, pin_dir[k].reserve(sizeof(vs_bgzf_member) * nm, sizeof(vs_bgzf_member) * (nm + nm / 4 + 64)));
            VS_HIP(ctx, pin_res[k].reserve(sizeof(uint32_t) * 4u * nm, sizeof(uint32_t) * 4u * (nm + nm / 4 + 64)));
            memcpy(pin_dir[k].ptr(), dir[k].data(), sizeof(vs_bgzf_member) * nm);
            if (int rc = reserve_n<vs_bgzf_member>(ctx, d_dir, nm)) return rc;
            if (int rc = reserve_n<uint32_t>(ctx, d_res, 4u * nm)) return rc;
            VS_HIP(ctx, hipMemcpyAsync(d_comp.as<uint8_t>(), pin[k].as<uint8_t>(), bytes, hipMemcpyHostToDevice, st));
            VS_HIP(ctx, hipMemcpyAsync(d_dir.as<vs_bgzf_member>(), pin_dir[k].ptr(), sizeof(vs_bgzf_member) * nm, hipMemcpyHostToDevice, st));
            VS_HIP(ctx, hipMemsetAsync(d_res.as<uint32_t>(), 0xFF, sizeof(uint32_t) * 4u * nm, st));
            vs_launch_inflate_count(st, d_comp.as<uint8_t>(), bytes, d_scratch.as<uint8_t>(), grid, d_dir.as<vs_bgzf_member>(), (uint32_t)nm, d_res.as<uint32_t>());
            VS_HIP(ctx, hipGetLastError());
            VS_HIP(ctx, hipMemcpyAsync(pin_res[k].ptr(), d_res.as<uint32_t>(), sizeof(uint32_t) * 4u * nm, hipMemcpyDeviceToHost, st));
        }
    }
    return VS_OK;
}

// Test aid: the device line scanner on host text.  ends[i] (cap of them) = byte offset of newline i; info[0] = newlines,
// info[1] = flags (1: '\r', 2: a byte >= 0x80), info[2] = the record cut: one past the newline that ends the last line
// completing a record when the text's first line has number `line0` (mod 4), 0 if none.
int vs_fastq_scan_text(vs_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t line0, uint64_t *ends, uint64_t cap, uint64_t info[3]) {
    if (!ctx || (!text && n) || !info || n > STREAM_MAX_WINDOW) return vs_fail(ctx, VS_E_ARG, "vs_fastq_scan_text: bad argument");
    VS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t words = (n + 15u) / 16u, wgs = (words + SL_TPB - 1u) / SL_TPB;
    VsDevBuf txt_buf, wg_buf, ends_buf, st_buf;
    uint32_t hs[ST_N] = {0};
    VS_HIP(ctx, txt_buf.reserve(words * 16u + 16u));
    VS_HIP(ctx, wg_buf.reserve(sizeof(uint32_t) * (wgs + 1u)));
    VS_HIP(ctx, ends_buf.reserve(sizeof(uint32_t) * (n + 1u)));
    VS_HIP(ctx, st_buf.reserve(sizeof(uint32_t) * ST_N));
    uint8_t *d_txt = txt_buf.as<uint8_t>();
    uint32_t *d_wg = wg_buf.as<uint32_t>(), *d_ends = ends_buf.as<uint32_t>(), *d_st = st_buf.as<uint32_t>();
    VS_HIP(ctx, hipMemsetAsync(d_st, 0, sizeof(uint32_t) * ST_N, st));
    if (n) VS_HIP(ctx, hipMemcpyAsync(d_txt, text, n, hipMemcpyHostToDevice, st));
    if (wgs) {
        hipLaunchKernelGGL(k_sl_count, dim3((unsigned)wgs), dim3(SL_TPB), 0, st, (const uint8_t *)d_txt, n, d_wg, d_st);
        hipLaunchKernelGGL(k_sl_scan, dim3(1), dim3(SL_SCAN_TPB), 0, st, d_wg, (uint32_t)wgs, d_st + ST_NL);
        hipLaunchKernelGGL(k_sl_scatter, dim3((unsigned)wgs), dim3(SL_TPB), 0, st, (const uint8_t *)d_txt, n, (const uint32_t *)d_wg, d_ends);
        VS_HIP(ctx, hipGetLastError());
    }
    VS_HIP(ctx, hipMemcpyAsync(hs, d_st, sizeof hs, hipMemcpyDeviceToHost, st));
    VS_HIP(ctx, hipStreamSynchronize(st));
    std::vector<uint32_t> h(hs[ST_NL] ? hs[ST_NL] : 1u);
    if (hs[ST_NL]) VS_HIP(ctx, hipMemcpy(h.data(), d_ends, sizeof(uint32_t) * hs[ST_NL], hipMemcpyDeviceToHost));
    const uint64_t nl = hs[ST_NL];
    info[0] = nl;
    info[1] = hs[ST_FLAGS];
    // newline i ends line line0 + i; a record closes with a line of number 3 mod 4
    const uint64_t first_close = (3u + 4u - (line0 & 3u)) & 3u;  // index of the first newline that closes a record
    info[2] = 0;
    if (nl > first_close) {
        const uint64_t last_close = first_close + (nl - 1u - first_close) / 4u * 4u;
        info[2] = (uint64_t)h[last_close] + 1u;
    }
    if (ends)
        for (uint64_t i = 0; i < nl && i < cap; i++) ends[i] = h[i];
    return VS_OK;
}

}  // extern "C"
