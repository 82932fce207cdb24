// The device side of ONE file of FASTQ text in a streamed ingest, shared by the two-file stream (vs_stream.hip) and the
// interleaved one (vs_interleaved.hip): the window and its line ends (DevFile), the launches of the line-end kernels, a slot
// appended in each form the Reader delivers, host text mode for a flagged window, and the wording of a compressed stream
// that the device rejected.  What the top of vs_stream.hip says about these holds for both streams.
#pragma once
#include "vs_stream_reader.h"
#include "vs_stream_window.h"

#define SL_TPB 256

// the line-end kernels (vs_stream.hip).  count: newlines per workgroup of SL_TPB 16-byte words into wg (wgs + 1 words), scanned
// in place; st[ST_NL] = their number, st[ST_FLAGS] |= FL_*, st[ST_LAST] = the last byte (st zeroed before).  scatter: the byte
// offset of every newline, in order, from the scanned wg.  Nothing is launched for an empty window.
void vs_launch_sl_count(hipStream_t st, const uint8_t *txt, uint64_t n, uint32_t *wg, uint32_t *stat);
void vs_launch_sl_scatter(hipStream_t st, const uint8_t *txt, uint64_t n, const uint32_t *wg, uint32_t *ends);

namespace {

// per-window status the line-end kernels write
enum { ST_NL = 0, ST_FLAGS = 1, ST_LAST = 2, ST_PER_FILE = 4 };
enum { FL_CR = 1u, FL_HIGH = 2u };

inline uint64_t sl_workgroups(uint64_t size) { return ((size + 15u) / 16u + SL_TPB - 1u) / SL_TPB; }

// The device side of one file: the window (vs_stream_window.h) and its line ends.
struct DevFile {
    DevWindow w;
    size_t validated = 0;  // [0, validated) is known to be valid UTF-8 (ASCII, or checked on the host)
    VsDevBuf ends, wg;     // uint32
    uint32_t n_nl = 0, flags = 0, last_byte = 0;
    uint64_t records = 0;  // complete records in the window
    uint64_t first_record = 0;  // file-wide number of the window's first record
    bool eof = false;      // the reader's last slot is in the window
    int err = VS_OK;       // first failure of this file (reported after the end of both, in file order)
    std::string err_msg;
    uint32_t pend[4] = {0, 0, 0, 0};  // (end-of-input check) bytes of a character cut by a chunk boundary
    uint32_t n_pend = 0;
    uint32_t slot_base = 0;  // BGZF: running index of the first member of the slot appended last
    // a member range (vs_fastq_stream_open_range): lines still to drop from the front; whether the range ends where the file does
    uint64_t skip = 0;
    bool to_file_end = true;

    // what a read-back of the status words says about the window (hs: the ST_PER_FILE words of this file)
    void take_status(const uint32_t *hs) {
        n_nl = hs[ST_NL];
        flags = hs[ST_FLAGS];
        last_byte = hs[ST_LAST];
        if (!flags) validated = w.size;
        // (a final line without a newline counts -- at the end of the FILE: where a member range ends earlier, the bytes behind
        // its last newline are the front of a line of the next rank)
        const uint64_t lines = (uint64_t)n_nl + ((eof && to_file_end && w.size && last_byte != '\n') ? 1u : 0u);
        records = lines / 4u;
    }
};

// Text mode on the host for a flagged window (see the top of vs_stream.hip): its bytes up to the last line end (all of them
// at the end of the file) are translated and checked, the rest -- a partial line -- stays as it is for the next chunk.
inline int translate_window(vs_ctx *ctx, DevFile &d, const std::string &path) {
    std::vector<uint8_t> buf(d.w.size);
    if (d.w.size) VS_HIP(ctx, hipMemcpy(buf.data(), d.w.data(), d.w.size, hipMemcpyDeviceToHost));
    size_t cut = d.w.size;
    if (!d.eof) {
        size_t lim = d.w.size;
        if (lim && buf[lim - 1] == '\r') lim--;  // ("\r\n" may straddle the chunks)
        cut = 0;
        for (size_t i = lim; i-- > 0;)
            if (buf[i] == '\n' || buf[i] == '\r') { cut = i + 1; break; }
    }
    if (d.validated < cut && !vs_utf8_range_ok(buf.data(), cut, d.validated, cut)) {
        d.err = VS_E_UTF8;
        d.err_msg = path + " holds bytes that are not valid UTF-8 (the reference's text-mode read raises UnicodeDecodeError)";
        return VS_E_UTF8;
    }
    std::vector<uint8_t> out;
    out.reserve(d.w.size);
    for (size_t i = 0; i < cut;) {
        const uint8_t c = buf[i];
        if (c == '\r') {
            out.push_back('\n');
            i += (i + 1 < cut && buf[i + 1] == '\n') ? 2u : 1u;
        } else if (c < 0x80u) {
            out.push_back(c);
            i++;
        } else {  // one character, one byte (seq_chars); checked above
            const uint32_t cl = vs_utf8_char_len(buf.data() + i, cut - i);
            out.push_back('?');
            i += cl ? cl : 1u;
        }
    }
    const size_t translated = out.size();
    out.insert(out.end(), buf.begin() + (ptrdiff_t)cut, buf.end());
    if (!out.empty()) VS_HIP(ctx, hipMemcpy(d.w.data(), out.data(), out.size(), hipMemcpyHostToDevice));
    d.w.size = out.size();
    d.validated = translated;
    return VS_OK;
}

// The device refused the plain gzip stream of the file (DevWindow::gz_status).  A regular file is read again through zlib, for
// the code in the words of the reader's zlib loop; a pipe cannot be read twice, its message names the device's status.
inline void gzip_failed(DevFile &d, const Reader &r) {
    const std::string &path = r.path;
    char msg[700];
    struct stat sb;
    d.err = VS_E_ARG;
    if (fstat(r.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        snprintf(msg, sizeof msg, "%s: not a complete gzip stream (device status %s)", path.c_str(), vs_gz_status_name(d.w.gz_status));
        d.err_msg = msg;
        return;
    }
    int code = Z_OK;  // zlib over the whole file, as the reader's loop runs it
    {
        std::vector<uint8_t> in(1u << 20), out(1u << 20);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        uint64_t at = 0;
        bool eof = false, done = false;
        if (inflateInit2(&zs, 15 + 16) != Z_OK) code = Z_MEM_ERROR;
        while (code == Z_OK && !done) {
            if (zs.avail_in == 0 && !eof) {
                const ssize_t got = pread(r.fd, in.data(), in.size(), (off_t)at);
                if (got <= 0) eof = true;
                else at += (uint64_t)got;
                zs.next_in = in.data();
                zs.avail_in = got > 0 ? (uInt)got : 0u;
            }
            zs.next_out = out.data();
            zs.avail_out = (uInt)out.size();
            int rc = inflate(&zs, Z_NO_FLUSH);
            if (rc == Z_STREAM_END) {
                if (zs.avail_in == 0 && !eof) continue;  // (look whether more members follow)
                if (zs.avail_in == 0 && eof) done = true;
                else if (inflateReset(&zs) != Z_OK) code = Z_DATA_ERROR;
                continue;
            }
            if (rc == Z_OK || (rc == Z_BUF_ERROR && (zs.avail_out == 0 || (zs.avail_in == 0 && !eof)))) {
                if (zs.avail_in == 0 && eof && zs.avail_out != 0) code = Z_DATA_ERROR;  // truncated stream
                continue;
            }
            code = rc == Z_BUF_ERROR ? Z_DATA_ERROR : rc;
        }
        inflateEnd(&zs);
    }
    if (code == Z_OK) {
        snprintf(msg, sizeof msg, "%s: the gzip stream was rejected on the device (status %s) but zlib accepts it", path.c_str(),
                 vs_gz_status_name(d.w.gz_status));
        d.err = VS_E_STATE;
    } else {
        snprintf(msg, sizeof msg, "%s: not a complete gzip stream (zlib code %d)", path.c_str(), code);
    }
    d.err_msg = msg;
}

// A slot of a plain gzip file decoded behind the window, or (sl == nullptr, while DevWindow::gz.more) one more round on the
// compressed bytes that the text cap of the round before held back: no slot is taken for it.
inline int append_gzip(vs_ctx *ctx, hipStream_t st, DevFile &d, const Reader &r, const Slot *sl) {
    if (int rc = d.w.append_gzip(ctx, st, sl, r.path.c_str())) return rc;
    if (d.w.gz_status && d.err == VS_OK) gzip_failed(d, r);
    d.eof = d.w.gzip_at_end();
    return VS_OK;
}

// a slot of the file appended to its window: its text uploaded, or its BGZF members uploaded and inflated there (*d_bad, on
// the device: the running index of the first member that failed)
inline int append_slot(vs_ctx *ctx, hipStream_t st, DevFile &d, const Reader &r, const Slot &sl, uint32_t *d_bad) {
    if (d.w.size + sl.text > STREAM_MAX_WINDOW)
        return vs_fail(ctx, VS_E_RANGE, "%s: a window of %llu bytes without a complete record", r.path.c_str(), (unsigned long long)(d.w.size + sl.text));
    if (sl.comp) d.slot_base = (uint32_t)d.w.members;
    if (sl.gz) return append_gzip(ctx, st, d, r, &sl);
    if (int rc = d.w.append(ctx, st, sl, d_bad, d.slot_base)) return rc;
    d.eof = sl.last;
    return VS_OK;
}

// the next slot of the file appended to its window (blocks until the reader has one); while held-back gzip runs are pending,
// those instead, and `taken` stays empty
inline int append_chunk(vs_ctx *ctx, hipStream_t st, DevFile &d, Reader &r, SlotLease &taken, uint32_t *d_bad) {
    if (d.w.gz.more) return append_gzip(ctx, st, d, r, nullptr);
    taken = SlotLease(r);
    return append_slot(ctx, st, d, r, *taken, d_bad);
}

// One BGZF member (its payload at pay) as a plain gzip member through zlib: true when zlib accepts it; else *code = what
// the reader's zlib loop reports for such a stream (cut off, or bytes behind its end: Z_DATA_ERROR).
inline bool zlib_accepts(const uint8_t *pay, const vs_bgzf_member &mb, int *code) {
    std::vector<uint8_t> gz = {0x1f, 0x8b, 0x08, 0, 0, 0, 0, 0, 0, 0xff};  // a 10-byte header, the payload, the trailer
    gz.insert(gz.end(), pay, pay + mb.in_len);
    for (uint32_t v : {mb.crc, mb.isize})
        for (int k = 0; k < 4; k++) gz.push_back((uint8_t)(v >> (8 * k)));
    std::vector<uint8_t> out(1u << 16);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    int rc = inflateInit2(&zs, 15 + 16);
    if (rc == Z_OK) {
        zs.next_in = gz.data();
        zs.avail_in = (uInt)gz.size();
        do {
            zs.next_out = out.data();
            zs.avail_out = (uInt)out.size();
            rc = inflate(&zs, Z_NO_FLUSH);
        } while (rc == Z_OK && (zs.avail_in != 0 || zs.avail_out == 0));
        const bool accepted = rc == Z_STREAM_END && zs.avail_in == 0;
        inflateEnd(&zs);
        if (accepted) return true;
        if (rc >= 0 || rc == Z_BUF_ERROR) rc = Z_DATA_ERROR;
    }
    *code = rc;
    return false;
}

// After a scan: did the device reject a member of the slot appended last (bad: the status word *d_bad read back, ~0u: none)?
// Then zlib inflates that member on the host and the file fails with zlib's code, in the words of the reader's zlib loop
// (true: the file has failed).
inline bool member_failed(DevFile &d, const Reader &r, const Slot &sl, uint32_t bad) {
    if (!sl.comp || bad == 0xFFFFFFFFu) return false;
    const uint32_t idx = bad - d.slot_base;
    char msg[700];
    if (d.err != VS_OK) return true;
    if (idx >= sl.n_members) {
        d.err = VS_E_STATE;
        d.err_msg = r.path + ": the device reported a BGZF member that is not of the slot it inflated";
        return true;
    }
    const vs_bgzf_member mb = slot_member(sl, idx);
    uint32_t dev_status = 0;
    (void)hipMemcpy(&dev_status, d.w.mstat.as<uint32_t>() + idx, sizeof dev_status, hipMemcpyDeviceToHost);
    int rc = Z_DATA_ERROR;
    if (zlib_accepts(sl.buf.as<uint8_t>() + mb.in_off, mb, &rc)) {
        snprintf(msg, sizeof msg, "%s: BGZF member %llu was rejected on the device (status %u) but zlib accepts it", r.path.c_str(),
                 (unsigned long long)(d.slot_base + idx), dev_status);
        d.err = VS_E_STATE;
        d.err_msg = msg;
        return true;
    }
    snprintf(msg, sizeof msg, "%s: not a complete gzip stream (zlib code %d)", r.path.c_str(), rc);
    d.err = VS_E_ARG;
    d.err_msg = msg;
    return true;
}

// the window after its first `cut` bytes (`records` records) have gone: the leftover to the front of the other buffer
inline int drop_front(vs_ctx *ctx, hipStream_t st, DevFile &d, size_t cut, uint64_t records) {
    if (int rc = d.w.keep_from(ctx, st, cut)) return rc;
    d.validated = d.validated > cut ? d.validated - cut : 0;
    d.records -= records;
    d.first_record += records;
    return VS_OK;
}

}  // namespace
