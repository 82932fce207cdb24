// One-file stream of UNPAIRED reads: the unpaired survivors of a trimmer (R1_unpaired.fq.gz of Trimmomatic, --unpaired1 of
// fastp), the merged reads of an overlapping library (fastp --merge, PEAR, BBMerge), streamed as vs_interleaved.hip streams
// one file -- one Reader, one DevWindow, so every form the Reader knows (plain, FIFO, gzip through zlib, BGZF and plain gzip
// inflated on the device) comes with it -- without the matching: every complete record is a read of its own.
// Per window (the leftover of the one before + the slot appended):
//   k_sl_count / k_sl_scan / k_sl_scatter   the line ends, as for the two-file stream (vs_stream_lines.h); a flagged window
//                                           ('\r', a byte >= 0x80) goes through host text mode first.
// A block of n reads from the cursor is a SINGLES block, cut by the block builder (vs_block_singles, vs_reads.hip) from the
// records cursor ..., every second end absent -- the layout vs_pe_count takes.  When the window's records are out it is cut behind the last of them; the
// partial record leads the next window.  A trailing partial record at the end of the file is dropped, as the reference drops
// it from either of its files (len(lines) // 4).
// The host reads back counts, the cut and status words; no record text.
#include <algorithm>
#include <string>

#include "vs_internal.h"
#include "vs_stream_lines.h"

namespace {

// status words of a stream (the first ST_PER_FILE are the line scanner's)
enum {
    SS_BLOCK = 4,  // the VS_BLK_ST words of the block builder
    SS_BAD = 8,    // the first BGZF member the device rejected (a running index), ~0u: none
    SS_ALL = 12
};

}  // namespace

struct vs_fastq_se : StreamState {  // (SS_ALL status words)
    int device = 0;
    hipStream_t st = nullptr;
    Reader rd;
    DevFile df;  // the one window, its line ends
    bool scanned = false;  // df describes the window: line ends scattered, records counted
    uint32_t rec_cur = 0;  // the first record of the scanned window not yet delivered
    VsDevBuf d_wcnt;
    uint64_t reads = 0, records = 0;
    uint32_t flags_seen = 0;
};

namespace {

// count + scan of the window: its line ends counted, flags, records (synchronises the stream)
int se_scan(vs_ctx *ctx, vs_fastq_se *s) {
    DevFile &d = s->df;
    VS_HIP(ctx, hipMemsetAsync(s->d_stat, 0, sizeof(uint32_t) * ST_PER_FILE, s->st));
    if (int rc = reserve_n<uint32_t>(ctx, d.wg, sl_workgroups(d.w.size) + 1u)) return rc;
    vs_launch_sl_count(s->st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), s->d_stat);
    VS_HIP(ctx, hipGetLastError());
    VS_HIP(ctx, hipMemcpyAsync(s->h_stat, s->d_stat, sizeof(uint32_t) * SS_ALL, hipMemcpyDeviceToHost, s->st));
    VS_HIP(ctx, hipStreamSynchronize(s->st));
    d.take_status(s->h_stat);
    s->flags_seen |= d.flags;
    return VS_OK;
}

// The next window: the records of the last one cut off, a slot appended, the line ends found.
// *end: nothing more comes (the stream is done or has failed; the code is returned).
int se_next_window(vs_ctx *ctx, vs_fastq_se *s, bool *end) {
    DevFile &d = s->df;
    hipStream_t st = s->st;
    *end = true;
    if (s->scanned) {
        if (d.eof) {  // the end of the input: the reader's failure, if it had one
            if (s->rd.err != VS_OK) return s->fail(ctx, s->rd.err, s->rd.err_msg);
            s->done = true;
            return VS_OK;
        }
        size_t cut = 0;
        const uint64_t out = d.records;
        if (out) {  // one past the line end that closes the last record (not the end of the file: that line end is a newline)
            uint32_t at = 0;
            VS_HIP(ctx, hipMemcpyAsync(&at, d.ends.as<uint32_t>() + (4u * (size_t)out - 1u), sizeof at, hipMemcpyDeviceToHost, st));
            VS_HIP(ctx, hipStreamSynchronize(st));
            cut = (size_t)at + 1u;
            if (cut > d.w.size) return s->fail(ctx, VS_E_STATE, s->rd.path + ": a line end beyond the window");
        }
        if (int rc = drop_front(ctx, st, d, cut, out)) return s->fail(ctx, rc, vs_last_error(ctx));
        s->scanned = false;
        s->rec_cur = 0;
    }
    {
        SlotLease taken;  // (goes back once the stream is synchronised: the upload is done)
        if (int rc = append_chunk(ctx, st, d, s->rd, taken, s->d_stat + SS_BAD)) return s->fail(ctx, rc, vs_last_error(ctx));
        if (int rc = se_scan(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
        if (taken) (void)member_failed(d, s->rd, *taken, s->h_stat[SS_BAD]);
    }
    if (d.err == VS_OK && d.flags && d.validated < d.w.size) {  // (text that arrived with this slot: host text mode)
        if (translate_window(ctx, d, s->rd.path) == VS_OK)
            if (int rc = se_scan(ctx, s)) return s->fail(ctx, rc, vs_last_error(ctx));
    }
    if (d.err != VS_OK) return s->fail(ctx, s->rd.err != VS_OK ? s->rd.err : d.err, s->rd.err != VS_OK ? s->rd.err_msg : d.err_msg);
    if (d.records > (1ull << 30)) return s->fail(ctx, VS_E_RANGE, s->rd.path + ": more than 2^30 records in one window");
    if (int rc = reserve_n<uint32_t>(ctx, d.ends, (size_t)d.n_nl + 1u)) return s->fail(ctx, rc, vs_last_error(ctx));
    vs_launch_sl_scatter(st, d.w.data(), (uint64_t)d.w.size, d.wg.as<uint32_t>(), d.ends.as<uint32_t>());
    VS_HIP(ctx, hipGetLastError());
    s->scanned = true;
    s->records += d.records;
    *end = false;
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_fastq_se_open(vs_ctx *ctx, const char *path, vs_fastq_se **out) {
    if (!ctx || !path || !out) return vs_fail(ctx, VS_E_ARG, "vs_fastq_se_open: bad argument");
    *out = nullptr;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    vs_fastq_se *s = new vs_fastq_se();
    s->device = ctx->device;
    Reader &r = s->rd;
    fastq_switches(r, false, s->df.w.gz.text_cap);
    if (int rc = r.open_file(ctx, path)) {
        delete s;
        return rc;
    }
    hipError_t e1 = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e1 == hipSuccess) e1 = s->reserve_stat(SS_ALL);
    if (e1 == hipSuccess) e1 = hipMemset(s->d_stat + SS_BAD, 0xFF, sizeof(uint32_t));
    if (e1 != hipSuccess) {
        vs_fastq_se_close(s);
        return vs_fail(ctx, VS_E_HIP, "vs_fastq_se_open: %s", hipGetErrorString(e1));
    }
    r.th = std::thread([rp = &s->rd] { rp->run(); });
    *out = s;
    return VS_OK;
}

int vs_fastq_se_next(vs_ctx *ctx, vs_fastq_se *s, uint64_t max_reads, vs_reads **out, uint64_t *n_reads) {
    if (!ctx || !s || !out || !n_reads) return vs_fail(ctx, VS_E_ARG, "vs_fastq_se_next: bad argument");
    *out = nullptr;
    *n_reads = 0;
    if (s->failed != VS_OK) return s->again(ctx);
    if (s->done) return VS_OK;
    VS_HIP(ctx, hipSetDevice(ctx->device));
    if (!max_reads || max_reads > (1ull << 30)) max_reads = 1ull << 30;
    DevFile &d = s->df;
    while (!s->scanned || s->rec_cur >= d.records) {
        bool end = false;
        const int rc = se_next_window(ctx, s, &end);
        if (end) return rc;
    }
    // ---- the block of n reads from the cursor
    const uint64_t n = std::min<uint64_t>(d.records - s->rec_cur, max_reads);
    const SlWin win = {d.w.data(), d.ends.as<const uint32_t>(), d.n_nl, (uint32_t)d.w.size};
    vs_reads *r = nullptr;
    const VsBlockJob job = {ctx, s->st, 2u * n, &s->d_wcnt, s->d_stat + SS_BLOCK, s->h_stat + SS_BLOCK, VS_BLK_ST, false};
    const hipError_t e1 = vs_block_singles(job, win, nullptr, s->rec_cur, &r);
    if (e1 != hipSuccess) return s->fail_hip(ctx, "vs_fastq_se_next", e1);
    if (!r)  // (a singles source faults no end: the end is over the limit)
        return s->fail(ctx, VS_E_RANGE, too_long_line(s->rd.path, d.first_record + s->rec_cur + ((s->h_stat[SS_BLOCK + VS_BLK_BAD] & ~VS_BLK_OVER) >> 1)));
    s->rec_cur += (uint32_t)n;
    s->reads += n;
    *out = r;
    *n_reads = n;
    return VS_OK;
}

int vs_fastq_se_info(const vs_fastq_se *s, uint64_t info[6]) {
    if (!s || !info) return VS_E_ARG;
    info[0] = s->reads;
    info[1] = s->records;
    info[2] = s->rd.text_bytes + s->df.w.gz.text;
    info[3] = s->rd.raw_bytes;
    info[4] = (uint64_t)s->flags_seen | (s->rd.gzip ? 4u : 0u) | (s->done ? 16u : 0u);
    info[5] = 0;
    return VS_OK;
}

void vs_fastq_se_close(vs_fastq_se *s) {
    if (!s) return;
    s->rd.shut();
    if (s->st) (void)hipStreamSynchronize(s->st);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

}  // extern "C"
